/*
 * is_k_conv_backward.hip -- f21, and f22's launcher: the backward pass of is_conv_bn at stride 1 (a 3x3 dilated or 1x1 convolution, folded
 * BatchNorm frozen at its running statistics, optional residual, optional ReLU): the masked gradient gh, dshift, the
 * transposed pack for dX, the weight-gradient partials G, their reduction to dW, and dscale.  dX itself is
 * is_k_conv3x3.hip's launch (isk_launch_conv_bn) on gh and the transposed pack; that file is not touched.
 *
 * Numerics contract: include/instance_stixels_core.h f21, DESIGN.md 10aa.  In short: gh is the half rounding of dY under the
 * ReLU mask of the STORED output; everything else is computed from gh.  dshift, Gsum, dW and dscale are binary64 sums in
 * an order the shape fixes; G's chunk partials are fp32 MFMA accumulators, one per (co, ci, tap) and chunk, fed in an
 * order the shape fixes.  No floating-point atomics; the same bytes on every run and for every choice of outputs.
 *
 * k_conv_bwd_weight<DT, TAPS>, the hot kernel: an implicit GEMM with M = channels_out, N = channels_in x taps, K = the
 * pixels of chunk (image, band of IS_CONV_BACKWARD_BAND rows).  Both operands have K contiguous in memory (pixels of a
 * row of an NCHW plane), which is the fragment of the 32x32x16 shapes as it is (lane l: row l & 31, k = 8 (l >> 5) + j);
 * neither needs a transpose.  For tap kx the x operand is shifted against gh by (kx - 1) d pixels, so a fragment read
 * straight from a row would start off 16-byte alignment.  That is solved in the staging: per kx the workgroup holds its
 * own copy of the x rows, shifted by (kx - 1) d, so that every fragment of every tap is one aligned ds_read_b128.
 *
 * Tile mapping.  A workgroup of four waves owns 64 co x 64 ci x all taps of one chunk; wave w takes the 32 x 32 block
 * (w & 1, w >> 1) with TAPS accumulators (144 registers at 3x3).  It walks segments of CB_SEG = 32 pixels (two K steps)
 * of the chunk's rows.  A step (one row y of one segment) multiplies
 *   A         gh[co0 .. co0 + 63][y][xs .. xs + 31]
 *   B ky, kx  x[ci0 .. ci0 + 63][y + (ky - 1) d][xs + (kx - 1) d .. + 31]
 * each a 4 KB tile.  The x tiles are staged ONCE PER kx, not per tap: the rows of a segment go by in residue classes
 * mod d (y = ya + res, ya + res + d, ...), so that the rows y - d, y, y + d of a step are the previous, this and the next
 * row of the class, held in a ring of three rows per kx copy.  A step stages gh and the one new row in its three kx
 * copies: 4 tiles (10 at the first step of a class) for 18 MFMAs per wave, where staging every tap's tile took 10.  A
 * pixel outside the image or past the row's end, and a channel past the last, is zero (the address is clamped into the
 * array and the loaded bits are masked: no select on a loaded value).  Channels that are no multiple of
 * 64 compute on zeros and are not stored.  Workgroup b is taken to run on XCD b & 7 (the round-robin dispatch k_conv3x3
 * relies on): the weight tiles of ONE chunk follow each other in that XCD's share of the grid, so that the chunk's gh
 * and x can come from memory once and from that XCD's L2 for the other tiles.  Reasoned, not measured: the tiles of a
 * chunk are 8 workgroups apart in the grid, and once more workgroups than are resident lie between them they are not
 * adjacent in time.
 *
 * LDS tile and its bank account (reasoned from the addresses, not measured).  A tile is [4 slots of 8 pixels][64 rows]
 * 16-byte entries; entry e(s, row) = 64 s + (row ^ 2 s).
 *   reads   ds_read_b128, lane (r, half) at K step ks reads entry e(2 ks + half, row0 + r).  A 16-lane group of that
 *           instruction holds 16 lanes of one half whose r are distinct mod 16 ({0-3, 12-15, 20-27}, {4-11, 16-19,
 *           28-31}); the XOR permutes inside an aligned group of 16 entries, so the group reads the 16 slots of one
 *           256-byte bank row: conflict-free.
 *   writes  ds_write_b32 of a pixel pair; a thread's item is (row, pair q), consecutive threads consecutive q.  Dword
 *           256 s + 4 (row ^ 2 s) + (q & 3) with s = q >> 2 (256 s is 0 mod the 32 banks): the 32 lanes of a half wave
 *           are rows 2 k and 2 k + 1 times 16 pairs; (row ^ 2 s) & 7 takes 8 distinct values over them, times 4 dwords: 32 distinct banks of the 32 that a
 *           write sees: conflict-free.
 * The global loads are 2-byte loads (the row bases are only 2-byte aligned when cols8 is odd), consecutive lanes
 * consecutive pixels.  The loads of a step are issued one step ahead into 32 registers and go to LDS between the two
 * barriers of their step, so they are in flight while the step before multiplies; a deeper pipeline is not built.
 */
#include "is_conv_backward.h"

#define CB_PREP_ITEMS 8            /* elements of a thread of k_conv_bwd_prepare */
#define CB_PREP_BLOCK (256 * CB_PREP_ITEMS)

/* The sum of the 256 threads' values in binary64: t += t + s for s = 128 .. 1.  `lds` holds 256 doubles; every thread
 * of the block calls, and gets the sum. */
__device__ __forceinline__ double cb_block_sum(double v, double* lds) {
    const int tid = threadIdx.x;
    __syncthreads(); /* (the previous use of lds is over) */
    lds[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) lds[tid] = lds[tid] + lds[tid + s];
        __syncthreads();
    }
    return lds[0];
}

/* gh and the dshift block sums.  Grid (blocks of a plane, co, n); a thread takes 8 consecutive elements of the plane.
 * vec: P % 8 == 0 and every base and stride keeps a thread's 8 elements 16-byte aligned (32 for an fp32 operand). */
template <int DT>
__global__ __launch_bounds__(256) void k_conv_bwd_prepare(const void* __restrict__ out_, int out_f32, int relu,
                                                          const void* __restrict__ dy_, int dy_f32, long long dy_stride,
                                                          uint16_t* __restrict__ gh, double* __restrict__ shift_part,
                                                          int Cout, int P, int vec) {
    __shared__ double lds[256];
    const int tid = threadIdx.x, co = blockIdx.y, n = blockIdx.z;
    const int e0 = blockIdx.x * CB_PREP_BLOCK + tid * CB_PREP_ITEMS;
    const size_t plane = ((size_t)n * Cout + co) * P;
    const size_t dplane = (size_t)n * (size_t)dy_stride + (size_t)co * P;
    float g[CB_PREP_ITEMS];
    uint16_t keep[CB_PREP_ITEMS];
    if (vec && e0 >= P) { /* (past the plane: +0 into the block's sum, nothing stored) */
#pragma unroll
        for (int j = 0; j < 8; ++j) g[j] = 0.0f, keep[j] = 0u;
    } else if (vec) { /* (P % 8 == 0: the 8 elements are inside together) */
        if (dy_f32) {
            const float4 a = *(const float4*)((const float*)dy_ + dplane + e0), b = *(const float4*)((const float*)dy_ + dplane + e0 + 4);
            g[0] = a.x, g[1] = a.y, g[2] = a.z, g[3] = a.w, g[4] = b.x, g[5] = b.y, g[6] = b.z, g[7] = b.w;
        } else {
            const uint4 q = *(const uint4*)((const uint16_t*)dy_ + dplane + e0);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) g[j] = cb_widen<DT>((uint16_t)(w[j >> 1] >> (16 * (j & 1))));
        }
        if (!relu) {
#pragma unroll
            for (int j = 0; j < 8; ++j) keep[j] = 0xffffu;
        } else if (out_f32) {
            const float4 a = *(const float4*)((const float*)out_ + plane + e0), b = *(const float4*)((const float*)out_ + plane + e0 + 4);
            const float o[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) keep[j] = o[j] > 0.0f ? 0xffffu : 0u;
        } else {
            const uint4 q = *(const uint4*)((const uint16_t*)out_ + plane + e0);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) keep[j] = cb_widen<DT>((uint16_t)(w[j >> 1] >> (16 * (j & 1)))) > 0.0f ? 0xffffu : 0u;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int e = min(e0 + j, P - 1); /* (past the plane: loaded in bounds, masked below) */
            g[j] = dy_f32 ? ((const float*)dy_)[dplane + e] : cb_widen<DT>(((const uint16_t*)dy_)[dplane + e]);
            float o = 1.0f;
            if (relu) o = out_f32 ? ((const float*)out_)[plane + e] : cb_widen<DT>(((const uint16_t*)out_)[plane + e]);
            keep[j] = (e0 + j < P && o > 0.0f) ? 0xffffu : 0u;
        }
    }
    uint16_t h[CB_PREP_ITEMS];
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        h[j] = cb_round<DT>(g[j]) & keep[j];
        s = s + (double)cb_widen<DT>(h[j]);
    }
    if (vec) {
        if (e0 < P) {
            uint4 q;
            q.x = h[0] | ((uint32_t)h[1] << 16), q.y = h[2] | ((uint32_t)h[3] << 16);
            q.z = h[4] | ((uint32_t)h[5] << 16), q.w = h[6] | ((uint32_t)h[7] << 16);
            *(uint4*)(gh + plane + e0) = q;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (e0 + j < P) gh[plane + e0 + j] = h[j];
    }
    if (shift_part) { /* (the same for the whole grid) */
        const double total = cb_block_sum(s, lds);
        if (tid == 0) shift_part[((size_t)n * Cout + co) * gridDim.x + blockIdx.x] = total;
    }
}

/* The transposed, tap-flipped, scaled pack in is_conv_pack_weights' layout for (channels_out' = Cin, channels_in' = Cout):
 * packed[((tile * chunks + chunk) * taps + t) * 512 + h * 256 + r * 8 + j] = round(scale[co] * w_half[co][ci][taps - 1 - t])
 * with ci = 32 tile + r, co = 16 chunk + 8 h + j; and the launch's scale 1 and shift 0, [Cin] each. */
template <int DT>
__global__ __launch_bounds__(256) void k_conv_bwd_pack_t(const float* __restrict__ weight, const float* __restrict__ scale,
                                                         uint16_t* __restrict__ packed, float* __restrict__ ones,
                                                         float* __restrict__ zeros, int Cin, int Cout, int taps, int total) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < Cin) ones[e] = 1.0f, zeros[e] = 0.0f;
    if (e >= total) return;
    const int j = e & 7, r = (e >> 3) & 31, h = (e >> 8) & 1, t = (e >> 9) % taps, blk = (e >> 9) / taps;
    const int chunks = Cout / 16, chunk = blk % chunks, tile = blk / chunks;
    const int ci = 32 * tile + r, co = 16 * chunk + 8 * h + j;
    const float wh = cb_widen<DT>(cb_round<DT>(weight[((size_t)co * Cin + ci) * taps + (taps - 1 - t)]));
    float product = scale[co] * wh;
    /* the fp32 product as a value: without this the compiler multiplies with v_fma_mixlo_f16, which rounds the exact
     * product to the half once and differs from round_half(fp32 product) in the double-rounding cases */
    asm volatile("" : "+v"(product));
    packed[e] = cb_round<DT>(product);
}

/* part[((chunk * TAPS + tap) * Cout + co) * Cin + ci], chunk = image * bands + band */
template <int DT, int TAPS>
__global__ __launch_bounds__(256) void k_conv_bwd_weight(const uint16_t* __restrict__ gh, const uint16_t* __restrict__ x,
                                                         float* __restrict__ part, int Cin, int Cout, int H, int W, int d_,
                                                         int bands, int tiles_ci, int tiles, int chunks) {
    static_assert(TAPS == 9 || TAPS == 1, "a 3x3 or a 1x1 convolution");
    const int d = TAPS == 1 ? 0 : d_;
    constexpr int KX = TAPS == 9 ? 3 : 1;
    extern __shared__ uint4 cb_lds[]; /* [1 + TAPS] tiles: gh, then x [ring slot][kx] */
    uint32_t* const ldsw = (uint32_t*)cb_lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, half = lane >> 5;
    /* workgroup b of the grid is taken to run on XCD b & 7: the weight tiles of a chunk follow each other there */
    const int seq = blockIdx.x >> 3, tile = seq % tiles, chunk = (seq / tiles) * 8 + (blockIdx.x & 7);
    if (chunk >= chunks) return; /* (the whole workgroup, before any barrier) */
    const int n = chunk / bands, ya = (chunk % bands) * IS_CONV_BACKWARD_BAND, yb = min(ya + IS_CONV_BACKWARD_BAND, H);
    const int co0 = (tile / tiles_ci) * 64, ci0 = (tile % tiles_ci) * 64;
    const int mrow = 32 * (wave & 1), nrow = 32 * (wave >> 1);
    const size_t plane = (size_t)H * W;
    const uint16_t* const ghn = gh + (size_t)n * Cout * plane;
    const uint16_t* const xn = x + (size_t)n * Cin * plane;

    cb_acc acc[TAPS];
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;

    /* 3x3: for a segment, the rows of the chunk go by in residue classes mod d: y = ya + res, ya + res + d, ...; step t
     * of a class needs the x rows t - 1, t, t + 1 of that class (image rows y - d, y, y + d), which stay in a ring of
     * three rows per kx copy: row j of the class lives in ring slot (j + 1) % 3.  The first step of a class stages rows
     * -1, 0 and 1, every later step row t + 1 alone, over the slot of row t - 2: 3 staged x tiles and gh per step. */
    const int classes = TAPS == 1 ? 1 : min(d, yb - ya), stride = TAPS == 1 ? 1 : d;

    /* A thread's four items (row, pixel pair q) of a tile.  The loads of a step go into registers one step ahead, raw; the
     * masks are applied to the bits when the registers go to LDS (no select on a loaded value). */
    auto load_a = [&](int y, uint32_t (&v)[4][2], int xs) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int idx = tid + 256 * it, row = idx >> 4, p = xs + 2 * (idx & 15);
            const uint16_t* src = ghn + (size_t)min(co0 + row, Cout - 1) * plane + (size_t)y * W;
            v[it][0] = src[min(p, W - 1)], v[it][1] = src[min(p + 1, W - 1)];
        }
    };
    auto store_a = [&](const uint32_t (&v)[4][2], int xs) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int idx = tid + 256 * it, row = idx >> 4, q = idx & 15, p = xs + 2 * q;
            const bool in_c = co0 + row < Cout;
            uint32_t k0 = in_c && p < W ? 0xffffu : 0u, k1 = in_c && p + 1 < W ? 0xffffu : 0u;
            asm volatile("" : "+v"(k0), "+v"(k1)); /* a mask on the bits, not a branch around the loads */
            ldsw[4 * cb_entry(q >> 2, row) + (q & 3)] = (v[it][0] & k0) | ((v[it][1] & k1) << 16);
        }
    };
    auto load_b = [&](int gy, uint32_t (&v)[4][KX][2], int xs) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int idx = tid + 256 * it, row = idx >> 4, p = xs + 2 * (idx & 15);
            const uint16_t* src = xn + (size_t)min(ci0 + row, Cin - 1) * plane + (size_t)min(max(gy, 0), H - 1) * W;
#pragma unroll
            for (int kx = 0; kx < KX; ++kx) {
                const int gx = p + (TAPS == 1 ? 0 : (kx - 1) * d);
                v[it][kx][0] = src[min(max(gx, 0), W - 1)], v[it][kx][1] = src[min(max(gx + 1, 0), W - 1)];
            }
        }
    };
    auto store_b = [&](int slot, int gy, const uint32_t (&v)[4][KX][2], int xs) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int idx = tid + 256 * it, row = idx >> 4, q = idx & 15, p = xs + 2 * q;
            const bool in_y = ci0 + row < Cin && gy >= 0 && gy < H;
#pragma unroll
            for (int kx = 0; kx < KX; ++kx) {
                const int gx = p + (TAPS == 1 ? 0 : (kx - 1) * d);
                uint32_t k0 = in_y && gx >= 0 && gx < W ? 0xffffu : 0u, k1 = in_y && gx + 1 >= 0 && gx + 1 < W ? 0xffffu : 0u;
                asm volatile("" : "+v"(k0), "+v"(k1));
                ldsw[4 * CB_TILE_ENTRIES * (1 + KX * slot + kx) + 4 * cb_entry(q >> 2, row) + (q & 3)] =
                    (v[it][kx][0] & k0) | ((v[it][kx][1] & k1) << 16);
            }
        }
    };

    uint32_t va[4][2], vb[4][KX][2];
    for (int xs = 0; xs < W; xs += CB_SEG) {
        for (int res = 0; res < classes; ++res) {
            const int y0 = ya + res; /* row j of the class is image row y0 + j d */
            __syncthreads(); /* the previous class's operands are no longer read */
            if (TAPS == 9) { /* rows -1 and 0 of the class, staged as they come; row 1 goes the common way */
                load_b(y0 - d, vb, xs), store_b(0, y0 - d, vb, xs);
                load_b(y0, vb, xs), store_b(1, y0, vb, xs);
            }
            load_a(y0, va, xs);
            load_b(TAPS == 9 ? y0 + d : y0, vb, xs);
            int t = 0;
            for (int y = y0; y < yb; y += stride, ++t) {
                if (t > 0) __syncthreads(); /* the previous step's operands are no longer read */
                store_a(va, xs);
                store_b(TAPS == 9 ? (t + 2) % 3 : 0, TAPS == 9 ? y + d : y, vb, xs);
                __syncthreads();
                if (y + stride < yb) { /* the next step's operands, in flight while this step multiplies */
                    load_a(y + stride, va, xs);
                    load_b(TAPS == 9 ? y + 2 * d : y + stride, vb, xs);
                }
                const int t3 = t % 3;
#pragma unroll
                for (int ks = 0; ks < CB_SEG / 16; ++ks) {
                    const int s = 2 * ks + half;
                    const uint4 a = cb_lds[cb_entry(s, mrow + r)];
                    const int eb = cb_entry(s, nrow + r);
#pragma unroll
                    for (int tap = 0; tap < TAPS; ++tap) { /* tap (ky, kx): row t + ky - 1 of the class, copy kx */
                        const int tile_b = TAPS == 1 ? 1 : 1 + KX * ((t3 + tap / 3) % 3) + tap % 3;
                        acc[tap] = cb_mfma<DT>(a, cb_lds[CB_TILE_ENTRIES * tile_b + eb], acc[tap]);
                    }
                }
            }
        }
    }

    /* register i of a lane is row (i & 3) + 8 (i >> 2) + 4 half of the wave's block (the C/D map of the 32x32 shapes) at
     * column r: 32 lanes store 32 consecutive ci */
    const int ci = ci0 + nrow + r;
#pragma unroll
    for (int tap = 0; tap < TAPS; ++tap)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int co = co0 + mrow + (i & 3) + 8 * (i >> 2) + 4 * half;
            if (co < Cout && ci < Cin) part[(((size_t)chunk * TAPS + tap) * Cout + co) * Cin + ci] = acc[tap][i];
        }
}

/* One thread per (tap, co, ci) of the partials' layout: Gsum in binary64 over the chunks in increasing order (image
 * outer, band inner), dW and Gsum in conv.weight's layout. */
__global__ __launch_bounds__(256) void k_conv_bwd_reduce(const float* __restrict__ part, int chunks, int Cin, int Cout,
                                                         int taps, const float* __restrict__ scale, float* __restrict__ dw,
                                                         double* __restrict__ gsum) {
    const int total = taps * Cout * Cin, idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    double s = 0.0;
#pragma unroll 8
    for (int c = 0; c < chunks; ++c) s = s + (double)part[(size_t)c * total + idx];
    const int ci = idx % Cin, co = (idx / Cin) % Cout, tap = idx / (Cin * Cout);
    const size_t at = ((size_t)co * Cin + ci) * taps + tap;
    if (dw) dw[at] = (float)((double)scale[co] * s);
    if (gsum) gsum[at] = s;
}

/* One block per co: dscale from Gsum and w_half, dshift from the block sums of k_conv_bwd_prepare; each a sum of
 * contiguous thread ranges in increasing index, then the LDS tree. */
template <int DT>
__global__ __launch_bounds__(256) void k_conv_bwd_channel(const double* __restrict__ gsum, const float* __restrict__ weight,
                                                          const double* __restrict__ shift_part, int n_images, int pblocks,
                                                          int Cin, int Cout, int taps, float* __restrict__ dscale,
                                                          float* __restrict__ dshift) {
    __shared__ double lds[256];
    const int tid = threadIdx.x, co = blockIdx.x;
    if (dscale) {
        const int items = Cin * taps, per = (items + 255) / 256;
        const size_t base = (size_t)co * items;
        double s = 0.0;
        for (int i = tid * per; i < min((tid + 1) * per, items); ++i)
            s = s + (double)cb_widen<DT>(cb_round<DT>(weight[base + i])) * gsum[base + i];
        const double total = cb_block_sum(s, lds);
        if (tid == 0) dscale[co] = (float)total;
    }
    if (dshift) {
        const long long items = (long long)n_images * pblocks, per = (items + 255) / 256;
        double s = 0.0;
        for (long long i = tid * per; i < min((tid + 1) * per, items); ++i) {
            const long long img = i / pblocks, blk = i % pblocks;
            s = s + shift_part[((size_t)img * Cout + co) * pblocks + blk];
        }
        const double total = cb_block_sum(s, lds);
        if (tid == 0) dshift[co] = (float)total;
    }
}

static size_t cb_align(size_t bytes) { return (bytes + 15) & ~(size_t)15; }
/* the bands of H OUTPUT rows: IS_CONV_BACKWARD_BAND rows at stride 1, IS_CONV_BACKWARD_STRIDE_BAND at stride 2 */
static int cb_bands(int H, int stride) {
    const int band = stride == 2 ? IS_CONV_BACKWARD_STRIDE_BAND : IS_CONV_BACKWARD_BAND;
    return (H + band - 1) / band;
}
static int cb_pblocks(int H, int W) { return (int)(((long long)H * W + CB_PREP_BLOCK - 1) / CB_PREP_BLOCK); }

/* the sections of the scratch, in this order, each 16-byte aligned */
struct cb_scratch {
    size_t gh, packed, ones, zeros, shift_part, gsum, part, end;
};
/* H, W: the OUTPUT's extents (the input's at stride 1) */
static cb_scratch cb_layout(int n, int Cin, int Cout, int H, int W, int kernel, int stride) {
    const size_t taps = (size_t)kernel * kernel, P = (size_t)H * W;
    cb_scratch s;
    s.gh = 0;
    s.packed = s.gh + cb_align((size_t)n * Cout * P * 2);
    s.ones = s.packed + cb_align((size_t)Cin * Cout * taps * 2);
    s.zeros = s.ones + cb_align((size_t)Cin * 4);
    s.shift_part = s.zeros + cb_align((size_t)Cin * 4);
    s.gsum = s.shift_part + cb_align((size_t)n * Cout * cb_pblocks(H, W) * 8);
    s.part = s.gsum + cb_align((size_t)Cout * Cin * taps * 8);
    s.end = s.part + cb_align((size_t)n * cb_bands(H, stride) * taps * Cout * Cin * 4);
    return s;
}

/* The grid of k_conv_bwd_weight (0: it does not fit 31 bits). */
static long long cb_weight_grid(int n, int Cin, int Cout, int H) {
    const long long tiles = (long long)((Cout + 63) / 64) * ((Cin + 63) / 64), chunks = (long long)n * cb_bands(H, 1);
    const long long grid = tiles * ((chunks + 7) / 8 * 8);
    return grid > 0x7fffffffLL ? 0 : grid;
}

extern "C" size_t isk_conv_backward_scratch_bytes(int n_images, int channels_in, int channels_out, int rows_in, int cols_in,
                                                  int kernel, int stride) {
    const int H = (rows_in + stride - 1) / stride, W = (cols_in + stride - 1) / stride;
    if (!(stride == 2 ? isk_conv_bwd_weight_s2_grid(n_images, channels_in, channels_out, H)
                      : cb_weight_grid(n_images, channels_in, channels_out, H)))
        return 0;
    return cb_layout(n_images, channels_in, channels_out, H, W, kernel, stride).end;
}

/* The arguments are checked by is_core.hip's conv_bn_backward_run, for is_conv_bn_backward and
 * is_conv_bn_stride_backward alike.  H, W: the OUTPUT's extents, which gh, dshift and the chunks go by. */
extern "C" hipError_t isk_launch_conv_bn_backward(const is_conv_bn_stride_backward_args* a, hipStream_t stream) {
    const int n = a->n_images, Cin = a->channels_in, Cout = a->channels_out, s2 = a->stride == 2;
    const int H = (a->rows_in + a->stride - 1) / a->stride, W = (a->cols_in + a->stride - 1) / a->stride;
    const int taps = a->kernel * a->kernel, P = H * W, pblocks = cb_pblocks(H, W), bands = cb_bands(H, a->stride), chunks = n * bands;
    const cb_scratch lay = cb_layout(n, Cin, Cout, H, W, a->kernel, a->stride);
    char* const scratch = (char*)a->d_scratch;
    uint16_t* const gh = a->d_grad_pre ? (uint16_t*)a->d_grad_pre : (uint16_t*)(scratch + lay.gh);
    uint16_t* const packed = (uint16_t*)(scratch + lay.packed);
    float* const ones = (float*)(scratch + lay.ones);
    float* const zeros = (float*)(scratch + lay.zeros);
    double* const shift_part = (double*)(scratch + lay.shift_part);
    double* const gsum = (double*)(scratch + lay.gsum);
    float* const part = (float*)(scratch + lay.part);
    const bool contract = a->d_grad_weight || a->d_grad_scale;
    const bool f16 = a->dtype == IS_HEAD_F16;
    if (!f16 && a->dtype != IS_HEAD_BF16) return hipErrorInvalidValue;
    if (a->kernel != 3 && a->kernel != 1) return hipErrorInvalidValue;

    {   /* gh, and the dshift block sums where dshift is asked for */
        const int out_f32 = a->out_dtype == IS_HEAD_F32, dy_f32 = a->grad_out_dtype == IS_HEAD_F32;
        /* a thread's 8 elements are one 16-byte access of a half operand, two of an fp32 one */
        const bool aligned = (uintptr_t)gh % 16 == 0 && (uintptr_t)a->d_grad_out % (dy_f32 ? 32 : 16) == 0 &&
                             (!a->relu || (uintptr_t)a->d_out % (out_f32 ? 32 : 16) == 0);
        const int vec = P % 8 == 0 && a->grad_image_stride % 8 == 0 && aligned;
        const dim3 grid(pblocks, Cout, n);
        double* const sp = a->d_grad_shift ? shift_part : nullptr;
        if (f16)
            hipLaunchKernelGGL(k_conv_bwd_prepare<IS_HEAD_F16>, grid, dim3(256), 0, stream, a->d_out, out_f32, a->relu,
                               a->d_grad_out, dy_f32, a->grad_image_stride, gh, sp, Cout, P, vec);
        else
            hipLaunchKernelGGL(k_conv_bwd_prepare<IS_HEAD_BF16>, grid, dim3(256), 0, stream, a->d_out, out_f32, a->relu,
                               a->d_grad_out, dy_f32, a->grad_image_stride, gh, sp, Cout, P, vec);
    }
    if (a->d_grad_features) { /* the transposed pack, then (stride 1) f18's launch with the channels swapped */
        const int total = Cin * Cout * taps;
        const dim3 grid((total + 255) / 256);
        if (f16)
            hipLaunchKernelGGL(k_conv_bwd_pack_t<IS_HEAD_F16>, grid, dim3(256), 0, stream, a->d_weight, a->d_scale, packed,
                               ones, zeros, Cin, Cout, taps, total);
        else
            hipLaunchKernelGGL(k_conv_bwd_pack_t<IS_HEAD_BF16>, grid, dim3(256), 0, stream, a->d_weight, a->d_scale, packed,
                               ones, zeros, Cin, Cout, taps, total);
        if (s2) { /* the gather form of the transposed convolution (is_k_conv_backward_stride.hip) */
            isk_launch_conv_bwd_data_s2(a, gh, packed, stream);
        } else {
            is_conv_bn_stride_args c = {};
            c.d_features = gh, c.dtype = a->dtype, c.n_images = n, c.channels_in = Cout, c.channels_out = Cin;
            c.rows_in = H, c.cols_in = W, c.kernel = a->kernel, c.stride = 1, c.dilation = a->dilation;
            c.d_packed = packed, c.d_scale = ones, c.d_shift = zeros, c.d_residual = a->d_grad_features_add, c.relu = 0;
            c.d_out = a->d_grad_features, c.out_dtype = a->grad_features_dtype;
            const hipError_t e = isk_launch_conv_bn(&c, stream);
            if (e != hipSuccess) return e;
        }
    }
    if (contract && s2) isk_launch_conv_bwd_weight_s2(a, gh, part, stream);
    if (contract && !s2) {
        const int tiles_ci = (Cin + 63) / 64, tiles = tiles_ci * ((Cout + 63) / 64);
        const dim3 grid((unsigned)cb_weight_grid(n, Cin, Cout, H));
        const size_t lds = (size_t)(1 + taps) * CB_TILE_ENTRIES * 16;
#define CB_WEIGHT(DT, TAPS)                                                                                          \
    hipLaunchKernelGGL((k_conv_bwd_weight<DT, TAPS>), grid, dim3(256), lds, stream, (const uint16_t*)gh,            \
                       (const uint16_t*)a->d_features, part, Cin, Cout, H, W, a->dilation, bands, tiles_ci, tiles, chunks)
        if (f16) {
            if (taps == 9) CB_WEIGHT(IS_HEAD_F16, 9); else CB_WEIGHT(IS_HEAD_F16, 1);
        } else {
            if (taps == 9) CB_WEIGHT(IS_HEAD_BF16, 9); else CB_WEIGHT(IS_HEAD_BF16, 1);
        }
#undef CB_WEIGHT
    }
    if (contract) {
        const int total = taps * Cout * Cin; /* at most 9 * 2^22 */
        hipLaunchKernelGGL(k_conv_bwd_reduce, dim3((total + 255) / 256), dim3(256), 0, stream, (const float*)part, chunks,
                           Cin, Cout, taps, a->d_scale, a->d_grad_weight, a->d_grad_scale ? gsum : nullptr);
    }
    if (a->d_grad_scale || a->d_grad_shift) {
        if (f16)
            hipLaunchKernelGGL(k_conv_bwd_channel<IS_HEAD_F16>, dim3(Cout), dim3(256), 0, stream, (const double*)gsum,
                               a->d_weight, (const double*)shift_part, n, pblocks, Cin, Cout, taps, a->d_grad_scale,
                               a->d_grad_shift);
        else
            hipLaunchKernelGGL(k_conv_bwd_channel<IS_HEAD_BF16>, dim3(Cout), dim3(256), 0, stream, (const double*)gsum,
                               a->d_weight, (const double*)shift_part, n, pblocks, Cin, Cout, taps, a->d_grad_scale,
                               a->d_grad_shift);
    }
    return hipGetLastError();
}

/* f23 (is_k_stem_backward.hip) runs the two reductions above on the stem's partials: the same kernels, the same
 * instantiations. */
extern "C" void isk_launch_conv_bwd_reduce(const float* part, int chunks, int Cin, int Cout, int taps, const float* scale,
                                           float* dw, double* gsum, hipStream_t stream) {
    const int total = taps * Cout * Cin;
    hipLaunchKernelGGL(k_conv_bwd_reduce, dim3((total + 255) / 256), dim3(256), 0, stream, part, chunks, Cin, Cout, taps,
                       scale, dw, gsum);
}

extern "C" void isk_launch_conv_bwd_channel(int dtype, const double* gsum, const float* weight, const double* shift_part,
                                            int n_images, int pblocks, int Cin, int Cout, int taps, float* dscale,
                                            float* dshift, hipStream_t stream) {
    if (dtype == IS_HEAD_F16)
        hipLaunchKernelGGL(k_conv_bwd_channel<IS_HEAD_F16>, dim3(Cout), dim3(256), 0, stream, gsum, weight, shift_part,
                           n_images, pblocks, Cin, Cout, taps, dscale, dshift);
    else
        hipLaunchKernelGGL(k_conv_bwd_channel<IS_HEAD_BF16>, dim3(Cout), dim3(256), 0, stream, gsum, weight, shift_part,
                           n_images, pblocks, Cin, Cout, taps, dscale, dshift);
}
