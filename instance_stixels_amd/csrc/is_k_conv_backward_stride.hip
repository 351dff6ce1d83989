/*
 * is_k_conv_backward_stride.hip -- f22: the two kernels that the backward pass of is_conv_bn_stride needs at stride 2
 * (kernel 3 with padding 1, or kernel 1; dilation 1): dX as the gather form of the transposed convolution, and the
 * weight-gradient partials G.  gh, dshift, the transposed pack, the reduction of the partials, dW and dscale are
 * is_k_conv_backward.hip's launches, and so is the launcher (isk_launch_conv_bn_backward), which calls the two
 * functions at the end of this file.  Numerics contract: include/instance_stixels_core.h f22, DESIGN.md 10ab.
 *
 * Extents: Hi x Wi is the input (x, dX), Ho x Wo = ceil(Hi / 2) x ceil(Wi / 2) the output (gh).
 *
 * k_conv_bwd_data_s2<DT, KERNEL>.  The cells, parity classes and tap table of the transposed convolution are
 * is_conv_backward.h's, at cb_parity_taps (kernel 1: the class (even, even) is w gh[Y][X] and the other three have no
 * tap).  A workgroup of four waves owns 32
 * ci x (4 x 32) cells, wave w the 32 cells of cell row Y0 + w.  Each class is its own chain of 32x32x16 MFMAs, M = ci, N =
 * the 32 cells, K = 16 co, in increasing 16-co chunk and, inside a chunk, increasing tap: one accumulator per dX
 * element, never split or combined.  Per 16-co chunk the workgroup stages the gh tile it reads, (4 + 1) rows x (32 + 1)
 * columns x 16 co, into LDS TRANSPOSED (co innermost), which is the B fragment: lane (cell r, half h) reads the 8 co
 * 8 h .. 8 h + 7 of its pixel as one ds_read_b128.  The A fragment is 16 bytes per lane straight from the transposed
 * pack (k_conv_bwd_pack_t's layout IS the fragment: 1 KB per (ci tile, chunk, tap), coalesced, from L2 after the first
 * workgroup).  The tile is double buffered: the next chunk's global loads are issued before this chunk's MFMAs and go
 * to the other buffer after them, one barrier per chunk.  A gh pixel outside the image is zero (address clamped, bits
 * masked: no select on a loaded value).  The epilogue adds features_add in fp32, rounds once and stores
 * a cell's two columns of a row as one 4-byte (half) or 8-byte (fp32) store where the row bases allow it: 32 lanes
 * write 128 (256) contiguous bytes.
 *
 * LDS account of the gh tile (reasoned from the addresses, not measured).  16-byte entry (h, row, col) at index
 * (h ROWS + row) COLS + col.
 *   reads   ds_read_b128: the 32 lanes of a half read 32 consecutive entries (col = r or r + 1), so any 16-lane group
 *           reads 256 consecutive bytes: every bank once, conflict-free, also from an odd start.
 *   writes  ds_write_b32 of a co pair; consecutive lanes are consecutive columns, 4 dwords apart: the 32 lanes of a
 *           half wave fall on 8 of the banks, a 4-way conflict.  Accepted: a thread writes 6 dwords per chunk against
 *           4 reads of 16 bytes and 9 MFMAs of 8 passes; coalesced global reads of whole rows were put first.
 *
 * k_conv_bwd_weight_s2<DT, TAPS> is the implicit GEMM that is_conv_backward.h describes (same tile, same LDS tile and bank
 * account, same fragment reads) at STEP = 2: the x operand of tap (ky, kx) is x[ci][2 y + ky - 1][2 p + kx - 1] for output
 * pixel (y, p), so the kx copies deinterleave the input row (kx = 1 is the even columns, kx = 0 and 2 the odd ones at p - 1
 * and p).  Output rows y and y + 1 share input row 2 y + 1: input row g lives in ring slot (g + 1) % 3, a step stages gh
 * and the two new rows 2 y and 2 y + 1 in their kx copies (7 tiles for 18 MFMAs per wave; stride 1 stages 4) and keeps
 * row 2 y - 1 from the step before.  A wave whose 32 x 32 block lies wholly past channels_out or channels_in (layer2's 16
 * channels in, a 1x1 with 32) skips its MFMAs and stores and only helps staging; a narrower tile is not built.
 * It shares cb_decode and cb_clear with k_conv_bwd_weight and KEEPS ITS OWN COPY of the staging, the MFMA step and the
 * epilogue (is_conv_backward.h's cb_load_* / cb_store_* at STEP = 2, CB_MULTIPLY, cb_store_part say the same): at 3x3 it
 * sits at the register limit (356 VGPRs, 12 SGPRs spilled to lanes), and through the shared functions the same work was
 * allocated differently (19 spills) and ran 1 % slower on layer2's shape.  Whoever changes one changes both.
 */
#include "is_conv_backward.h"

#define CS_CELL_ROWS 4   /* cell rows of a workgroup of k_conv_bwd_data_s2: one per wave */
#define CS_CELL_COLS 32  /* cells of a wave: N of the MFMA */

template <int DT, int KERNEL>
__global__ __launch_bounds__(256) void k_conv_bwd_data_s2(const uint16_t* __restrict__ gh, const uint4* __restrict__ packed,
                                                          const uint16_t* __restrict__ add, void* __restrict__ dx_,
                                                          int dx_f32, int pairs, int n_images, int Cin, int Cout, int Hi,
                                                          int Wi, int Ho, int Wo) {
    static_assert(KERNEL == 3 || KERNEL == 1, "a 3x3 or a 1x1 convolution");
    constexpr int HALO = KERNEL == 3 ? 1 : 0, ROWS = CS_CELL_ROWS + HALO, COLS = CS_CELL_COLS + HALO;
    constexpr int TAPS = KERNEL * KERNEL, ENTRIES = 2 * ROWS * COLS, ITEMS = 8 * ROWS * COLS, ITERS = (ITEMS + 255) / 256;
    __shared__ uint4 tile[2 * ENTRIES];
    uint32_t* const tilew = (uint32_t*)tile;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, half = lane >> 5;
    const int X0 = blockIdx.x * CS_CELL_COLS, Y0 = blockIdx.y * CS_CELL_ROWS;
    const int tiles_ci = Cin / 32, chunks = Cout / 16;
    const size_t plane_o = (size_t)Ho * Wo, plane_i = (size_t)Hi * Wi;

    for (int z = blockIdx.z; z < n_images * tiles_ci; z += gridDim.z) { /* (the same trip count for the whole workgroup) */
        const int n = z / tiles_ci, tile_ci = z % tiles_ci;
        const uint16_t* const ghn = gh + (size_t)n * Cout * plane_o;
        hm_acc16 acc[4]; /* (even, even), (even, odd), (odd, even), (odd, odd) */
        cb_clear(acc);

        /* A thread's items (co pair q, row, col) of the tile, consecutive threads consecutive columns. */
        uint32_t v[ITERS][2];
        auto load_tile = [&](int chunk) {
#pragma unroll
            for (int it = 0; it < ITERS; ++it) {
                const int item = min(tid + 256 * it, ITEMS - 1);
                const int col = item % COLS, row = (item / COLS) % ROWS, q = item / (COLS * ROWS);
                const uint16_t* src = ghn + (size_t)(16 * chunk + 2 * q) * plane_o + (size_t)min(Y0 + row, Ho - 1) * Wo +
                                      min(X0 + col, Wo - 1);
                v[it][0] = src[0], v[it][1] = src[plane_o];
            }
        };
        auto store_tile = [&](int buf) {
#pragma unroll
            for (int it = 0; it < ITERS; ++it) {
                const int item = tid + 256 * it, col = item % COLS, row = (item / COLS) % ROWS, q = item / (COLS * ROWS);
                uint32_t k = Y0 + row < Ho && X0 + col < Wo ? 0xffffu : 0u;
                asm volatile("" : "+v"(k)); /* a mask on the bits, not a branch around the loads */
                if (item < ITEMS)
                    tilew[4 * (ENTRIES * buf + ((q >> 2) * ROWS + row) * COLS + col) + (q & 3)] =
                        (v[it][0] & k) | ((v[it][1] & k) << 16);
            }
        };

        __syncthreads(); /* (the previous z's tiles are no longer read) */
        load_tile(0);
        store_tile(0);
        __syncthreads();
        for (int chunk = 0; chunk < chunks; ++chunk) {
            if (chunk + 1 < chunks) load_tile(chunk + 1); /* in flight while this chunk multiplies */
            const uint4* const wfrag = packed + ((size_t)(tile_ci * chunks + chunk) * TAPS) * 64 + lane;
            const uint4* const b = tile + ENTRIES * (chunk & 1) + (half * ROWS + wave) * COLS + r;
            /* the pack holds tap t at index TAPS - 1 - t (it is f18's flipped operand) */
            if (KERNEL == 3) {
                const uint4 bq[4] = {b[0], b[1], b[COLS], b[COLS + 1]};
                cb_parity_taps<DT>(acc, bq, [&](int t) { return wfrag[(TAPS - 1 - t) * 64]; });
            } else {
                acc[0] = hm_mfma<DT>(wfrag[0], b[0], acc[0]);
            }
            if (chunk + 1 < chunks) store_tile((chunk + 1) & 1);
            __syncthreads();
        }

        /* register i of a lane is ci row hm_cd_row(i, half) of the tile at cell X0 + r */
        const int Y = Y0 + wave, X = X0 + r, c0 = 2 * X;
        if (Y < Ho && X < Wo) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int ci = 32 * tile_ci + hm_cd_row(i, half);
#pragma unroll
                for (int pr = 0; pr < 2; ++pr) {
                    const int row = 2 * Y + pr;
                    if (row >= Hi) continue;
                    const size_t at = ((size_t)n * Cin + ci) * plane_i + (size_t)row * Wi + c0;
                    float v0 = acc[2 * pr][i], v1 = acc[2 * pr + 1][i];
                    const bool second = c0 + 1 < Wi;
                    if (pairs) { /* Wi is even and every base 4-byte (fp32: 8-byte) aligned: the cell's two columns at once */
                        if (add) {
                            const uint32_t a2 = *(const uint32_t*)(add + at);
                            v0 = v0 + hm_widen<DT>((uint16_t)a2), v1 = v1 + hm_widen<DT>((uint16_t)(a2 >> 16));
                        }
                        if (dx_f32) *(float2*)((float*)dx_ + at) = make_float2(v0, v1);
                        else *(uint32_t*)((uint16_t*)dx_ + at) = hm_round<DT>(v0) | ((uint32_t)hm_round<DT>(v1) << 16);
                    } else {
                        if (add) {
                            v0 = v0 + hm_widen<DT>(add[at]);
                            if (second) v1 = v1 + hm_widen<DT>(add[at + 1]);
                        }
                        if (dx_f32) {
                            ((float*)dx_)[at] = v0;
                            if (second) ((float*)dx_)[at + 1] = v1;
                        } else {
                            ((uint16_t*)dx_)[at] = hm_round<DT>(v0);
                            if (second) ((uint16_t*)dx_)[at + 1] = hm_round<DT>(v1);
                        }
                    }
                }
            }
        }
    }
}

/* part[((chunk * TAPS + tap) * Cout + co) * Cin + ci], chunk = image * bands + band of IS_CONV_BACKWARD_STRIDE_BAND
 * OUTPUT rows: k_conv_bwd_reduce's layout. */
template <int DT, int TAPS>
__global__ __launch_bounds__(256) void k_conv_bwd_weight_s2(const uint16_t* __restrict__ gh, const uint16_t* __restrict__ x,
                                                            float* __restrict__ part, int Cin, int Cout, int Hi, int Wi,
                                                            int Ho, int Wo, int bands, int tiles_ci, int tiles, int chunks) {
    static_assert(TAPS == 9 || TAPS == 1, "a 3x3 or a 1x1 convolution");
    constexpr int KX = TAPS == 9 ? 3 : 1, NEW = TAPS == 9 ? 2 : 1; /* kx copies of a row; new input rows of a step */
    extern __shared__ uint4 cs_lds[]; /* [1 + TAPS] tiles: gh, then x [ring slot][kx] */
    uint32_t* const ldsw = (uint32_t*)cs_lds;
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, half = lane >> 5;
    const cb_group g = cb_decode<IS_CONV_BACKWARD_STRIDE_BAND>(Ho, bands, tiles_ci, tiles);
    if (g.chunk >= chunks) return; /* (the whole workgroup, before any barrier) */
    const int chunk = g.chunk, n = g.n, ya = g.ya, yb = g.yb, co0 = g.co0, ci0 = g.ci0, mrow = g.mrow, nrow = g.nrow;
    const bool live = co0 + mrow < Cout && ci0 + nrow < Cin; /* (per wave) a block wholly past the channels multiplies nothing */
    const size_t plane_o = (size_t)Ho * Wo, plane_i = (size_t)Hi * Wi;
    const uint16_t* const ghn = gh + (size_t)n * Cout * plane_o;
    const uint16_t* const xn = x + (size_t)n * Cin * plane_i;

    hm_acc16 acc[TAPS];
    cb_clear(acc);

    /* column of the input that output pixel p reads in copy kx */
    auto col_of = [](int p, int kx) { return TAPS == 9 ? 2 * p + kx - 1 : 2 * p; };
    /* A thread's four items (row, pixel pair q) of a tile, as in k_conv_bwd_weight: raw loads one step ahead, masks on
     * the bits when the registers go to LDS. */
    auto load_a = [&](int y, uint32_t (&v)[4][2], int xs) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int idx = tid + 256 * it, row = idx >> 4, p = xs + 2 * (idx & 15);
            const uint16_t* src = ghn + (size_t)min(co0 + row, Cout - 1) * plane_o + (size_t)y * Wo;
            v[it][0] = src[min(p, Wo - 1)], v[it][1] = src[min(p + 1, Wo - 1)];
        }
    };
    auto store_a = [&](const uint32_t (&v)[4][2], int xs) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int idx = tid + 256 * it, row = idx >> 4, q = idx & 15, p = xs + 2 * q;
            const bool in_c = co0 + row < Cout;
            uint32_t k0 = in_c && p < Wo ? 0xffffu : 0u, k1 = in_c && p + 1 < Wo ? 0xffffu : 0u;
            asm volatile("" : "+v"(k0), "+v"(k1)); /* a mask on the bits, not a branch around the loads */
            ldsw[4 * cb_entry(q >> 2, row) + (q & 3)] = (v[it][0] & k0) | ((v[it][1] & k1) << 16);
        }
    };
    auto load_b = [&](int gy, uint32_t (&v)[4][KX][2], int xs) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int idx = tid + 256 * it, row = idx >> 4, p = xs + 2 * (idx & 15);
            const uint16_t* src = xn + (size_t)min(ci0 + row, Cin - 1) * plane_i + (size_t)min(max(gy, 0), Hi - 1) * Wi;
#pragma unroll
            for (int kx = 0; kx < KX; ++kx) {
                const int gx = col_of(p, kx);
                v[it][kx][0] = src[min(max(gx, 0), Wi - 1)], v[it][kx][1] = src[min(max(gx + 2, 0), Wi - 1)];
            }
        }
    };
    auto store_b = [&](int slot, int gy, const uint32_t (&v)[4][KX][2], int xs) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int idx = tid + 256 * it, row = idx >> 4, q = idx & 15, p = xs + 2 * q;
            const bool in_y = ci0 + row < Cin && gy >= 0 && gy < Hi;
#pragma unroll
            for (int kx = 0; kx < KX; ++kx) {
                const int gx = col_of(p, kx);
                uint32_t k0 = in_y && gx >= 0 && gx < Wi ? 0xffffu : 0u, k1 = in_y && gx + 2 >= 0 && gx + 2 < Wi ? 0xffffu : 0u;
                asm volatile("" : "+v"(k0), "+v"(k1));
                ldsw[4 * CB_TILE_ENTRIES * (1 + KX * slot + kx) + 4 * cb_entry(q >> 2, row) + (q & 3)] =
                    (v[it][kx][0] & k0) | ((v[it][kx][1] & k1) << 16);
            }
        }
    };
    /* ring slot of input row g (g >= -1) */
    auto slot_of = [](int g) { return TAPS == 9 ? (g + 1) % 3 : 0; };

    uint32_t va[4][2], vb[NEW][4][KX][2];
    for (int xs = 0; xs < Wo; xs += CB_SEG) {
        __syncthreads(); /* the previous segment's operands are no longer read */
        if (TAPS == 9) { /* input row 2 ya - 1, staged as it comes; every step keeps its last row for the next */
            load_b(2 * ya - 1, vb[0], xs), store_b(slot_of(2 * ya - 1), 2 * ya - 1, vb[0], xs);
        }
        load_a(ya, va, xs);
#pragma unroll
        for (int j = 0; j < NEW; ++j) load_b(2 * ya + j, vb[j], xs);
        for (int y = ya; y < yb; ++y) {
            if (y > ya) __syncthreads(); /* the previous step's operands are no longer read */
            store_a(va, xs);
#pragma unroll
            for (int j = 0; j < NEW; ++j) store_b(slot_of(2 * y + j), 2 * y + j, vb[j], xs);
            __syncthreads();
            if (y + 1 < yb) { /* the next step's operands, in flight while this step multiplies */
                load_a(y + 1, va, xs);
#pragma unroll
                for (int j = 0; j < NEW; ++j) load_b(2 * y + 2 + j, vb[j], xs);
            }
            if (live) {
                const int s0 = slot_of(2 * y - 1); /* tap (ky, kx): input row 2 y + ky - 1, copy kx */
#pragma unroll
                for (int ks = 0; ks < CB_SEG / 16; ++ks) {
                    const int s = 2 * ks + half;
                    const uint4 a = cs_lds[cb_entry(s, mrow + r)];
                    const int eb = cb_entry(s, nrow + r);
#pragma unroll
                    for (int tap = 0; tap < TAPS; ++tap) {
                        const int tile_b = TAPS == 1 ? 1 : 1 + KX * ((s0 + tap / 3) % 3) + tap % 3;
                        acc[tap] = hm_mfma<DT>(a, cs_lds[CB_TILE_ENTRIES * tile_b + eb], acc[tap]);
                    }
                }
            }
        }
    }

    /* register i of a lane is row (i & 3) + 8 (i >> 2) + 4 half of the wave's block at column r: 32 lanes store 32
     * consecutive ci */
    const int ci = ci0 + nrow + r;
    if (live) {
#pragma unroll
        for (int tap = 0; tap < TAPS; ++tap)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int co = co0 + mrow + (i & 3) + 8 * (i >> 2) + 4 * half;
                if (co < Cout && ci < Cin) part[(((size_t)chunk * TAPS + tap) * Cout + co) * Cin + ci] = acc[tap][i];
            }
    }
}

/* dX of a stride-2 call: every element of d_grad_features is written.  gh: [n][Cout][Ho][Wo]; packed: the transposed
 * pack of k_conv_bwd_pack_t, 16-byte aligned. */
extern "C" void isk_launch_conv_bwd_data_s2(const is_conv_bn_stride_backward_args* a, const void* gh, const void* packed,
                                            hipStream_t stream) {
    const int Hi = a->rows_in, Wi = a->cols_in, Ho = (Hi + 1) / 2, Wo = (Wi + 1) / 2, tiles_ci = a->channels_in / 32;
    const int dx_f32 = a->grad_features_dtype == IS_HEAD_F32;
    /* a cell's two columns in one access: every row base keeps the pair aligned */
    const int pairs = Wi % 2 == 0 && (uintptr_t)a->d_grad_features % (dx_f32 ? 8 : 4) == 0 &&
                      (uintptr_t)a->d_grad_features_add % 4 == 0;
    const long long zs = (long long)a->n_images * tiles_ci;
    const dim3 grid((Wo + CS_CELL_COLS - 1) / CS_CELL_COLS, (Ho + CS_CELL_ROWS - 1) / CS_CELL_ROWS,
                    (unsigned)(zs < 65535 ? zs : 65535));
    hm_dispatch(a->dtype, [&](auto dt) {
        hm_either<3, 1>(a->kernel == 3, [&](auto k) {
            hipLaunchKernelGGL((k_conv_bwd_data_s2<dt(), k()>), grid, dim3(256), 0, stream, (const uint16_t*)gh,
                               (const uint4*)packed, (const uint16_t*)a->d_grad_features_add, a->d_grad_features, dx_f32, pairs,
                               a->n_images, a->channels_in, a->channels_out, Hi, Wi, Ho, Wo);
        });
    });
}

/* The chunk partials of a stride-2 call into `part`. */
extern "C" void isk_launch_conv_bwd_weight_s2(const is_conv_bn_stride_backward_args* a, const void* gh, float* part,
                                              hipStream_t stream) {
    const int Cin = a->channels_in, Cout = a->channels_out, Hi = a->rows_in, Wi = a->cols_in;
    const int Ho = (Hi + 1) / 2, Wo = (Wi + 1) / 2;
    const int taps = a->kernel * a->kernel, bands = cb_bands(Ho, 2), chunks = a->n_images * bands;
    const int tiles_ci = (Cin + 63) / 64, tiles = tiles_ci * ((Cout + 63) / 64);
    const dim3 grid((unsigned)cb_weight_grid(a->n_images, Cin, Cout, bands));
    hm_dispatch(a->dtype, [&](auto dt) {
        hm_either<9, 1>(taps == 9, [&](auto t) {
            hipLaunchKernelGGL((k_conv_bwd_weight_s2<dt(), t()>), grid, dim3(256), cb_weight_lds(taps), stream,
                               (const uint16_t*)gh, (const uint16_t*)a->d_features, part, Cin, Cout, Hi, Wi, Ho, Wo, bands,
                               tiles_ci, tiles, chunks);
        });
    });
}
