/* is_k_unary.hip -- the unary column DP.  See is_kernels.h. */
#include "is_unary.h"

/* ====================================================================================== */
/* A7-A9  unary DP: one workgroup = (column, 64-row tile)                                  */
/* ====================================================================================== */
/* One (vB, vT) evaluation of the unary model (UnaryBest, unary_update: is_unary.h): the record of vB is a scalar
 * record, the vB side of the object data term comes out of the wave's lutT row (pick_lut).
 *   FAST  a column of the FAST encoding, walked DOWNWARDS with the `<=` update (below); the generic encoding is
 *         walked upwards with the reference's strict `<`.  The terms are returned for the bounds of the FAST walk. */
template <bool FAST, bool HAS_INVALID, bool SKY, bool DIAG, bool FIRST, int NR, bool NOGROUND = false>
__device__ __forceinline__ SegTerms unary_step(const DevParams& P, const RowRec& my, const RowRec& rb,
                                               const LutRow<NR>& lrow, const float* my_tile,
                                               const float* s_rcp, int vT, int vTc, int vhor, int vB,
                                               float hf_full, bool row_ok, UnaryBest& b) {
    const int h = vTc + 1 - vB;
    const bool live = DIAG ? ((h > 0) && row_ok) : row_ok;
    const int hc = DIAG ? max(h, 1) : h;
    const float r = s_rcp[hc]; /* RN(1/h) = (float)(1./h) = inverse_height, :485, :608 */
    /* full steps: the caller carries the height as a float (one 2-cycle subtraction per step
     * instead of an integer update plus a conversion; integers < 2^24 are exact) */
    const float hf = (DIAG || FIRST) ? (float)hc : hf_full;
    const SegTerms t = eval_segment<FAST, HAS_INVALID>(my, rb, hf, r, P.D, P.iw);
    const float od = my_tile[t.fni] - pick_lut<NR>(lrow, t.fni);
    unary_update<FAST, SKY, DIAG, FIRST, NOGROUND>(P, t, od, P.pw * r, vB, live, vT <= vhor, b);
    return t;
}

template <bool HAS_INVALID, bool SKY, bool DIAG, int NR, bool NOGROUND = false>
__device__ __forceinline__ int unary_range(const DevParams& P, const RowRec& my,
                                           const RowRec* __restrict__ rcol,
                                           const float* __restrict__ lcol, const float* my_tile,
                                           const float* s_rcp, int vT, int vTc, int vhor, int vB,
                                           int nw, int bound, bool row_ok, int lane4,
                                           __amdgpu_buffer_rsrc_t lrsrc, LutRow<NR>& next_row,
                                           UnaryBest& b) {
    float hf = (float)(vTc + 1 - vB);
    const float nwf = (float)nw;
    for (; vB <= bound; vB += nw) {
        const RowRec cur = sload_rec(rcol + vB);
        const LutRow<NR> row = next_row;
        load_lut_row<NR>(next_row, lrsrc, lcol, min(vB + nw, P.H), P.D, lane4); /* row H exists */
        unary_step<false, HAS_INVALID, SKY, DIAG, false, NR, NOGROUND>(P, my, cur, row, my_tile, s_rcp, vT, vTc,
                                                                       vhor, vB, hf, row_ok, b);
        hf -= nwf;
    }
    return vB;
}

/* The wave walks vB = w, w+nw, ... <= vB_end in ascending order through (at most) four ranges:
 * ground/full, ground/diagonal, sky/full, sky/diagonal (ground while vB <= vhor; "full" while
 * every lane of the tile has vT >= vB, i.e. vB <= tile_lo). */
template <bool HAS_INVALID, int NR>
__device__ __forceinline__ void unary_loop(const DevParams& P, const RowRec& my,
                                           const RowRec* __restrict__ rcol,
                                           const float* __restrict__ lcol, const float* my_tile,
                                           const float* s_rcp, int vT, int vTc, int vhor, int w,
                                           int nw, int tile_lo, int vB_end, int lane4,
                                           __amdgpu_buffer_rsrc_t lrsrc, UnaryBest& b) {
    const bool row_ok = vT < P.H;
    int vB = w;
    if (vB > vB_end) return;
    LutRow<NR> next_row; /* lutT row of the step that comes next */
    load_lut_row<NR>(next_row, lrsrc, lcol, vB, P.D, lane4);
    if (vB == 0) { /* first segment (:481-594): ground + object */
        const RowRec cur = sload_rec(rcol);
        const LutRow<NR> row = next_row;
        load_lut_row<NR>(next_row, lrsrc, lcol, min(nw, P.H), P.D, lane4);
        if (tile_lo == 0)
            unary_step<false, HAS_INVALID, false, true, true, NR>(P, my, cur, row, my_tile, s_rcp, vT, vTc, vhor,
                                                                  0, 0.0f, row_ok, b);
        else
            unary_step<false, HAS_INVALID, false, false, true, NR>(P, my, cur, row, my_tile, s_rcp, vT, vTc, vhor,
                                                                   0, 0.0f, row_ok, b);
        vB += nw;
    }
    if (tile_lo >= vhor) /* whole tile at / above the horizon */
        vB = unary_range<HAS_INVALID, false, false, NR, true>(
            P, my, rcol, lcol, my_tile, s_rcp, vT, vTc, vhor, vB, nw, min(min(vhor, tile_lo), vB_end),
            row_ok, lane4, lrsrc, next_row, b);
    else
        vB = unary_range<HAS_INVALID, false, false, NR>(P, my, rcol, lcol, my_tile, s_rcp, vT, vTc, vhor, vB, nw,
                                                        min(min(vhor, tile_lo), vB_end), row_ok, lane4, lrsrc,
                                                        next_row, b);
    vB = unary_range<HAS_INVALID, false, true, NR>(P, my, rcol, lcol, my_tile, s_rcp, vT, vTc, vhor, vB, nw,
                                                   min(vhor, vB_end), row_ok, lane4, lrsrc, next_row, b);
    vB = unary_range<HAS_INVALID, true, false, NR>(P, my, rcol, lcol, my_tile, s_rcp, vT, vTc, vhor, vB, nw,
                                                   min(tile_lo, vB_end), row_ok, lane4, lrsrc, next_row, b);
    unary_range<HAS_INVALID, true, true, NR>(P, my, rcol, lcol, my_tile, s_rcp, vT, vTc, vhor, vB, nw, vB_end, row_ok,
                                             lane4, lrsrc, next_row, b);
}


/* ====================================================================================== */
/* FAST columns: descending vB with an exact branch-and-bound (DESIGN.md "Pruning")        */
/* ====================================================================================== */
/* A wave walks its vB values DOWNWARDS.  After a full step at vB, every candidate vB' <= vB of
 * lane vT costs at least
 *     LB_o = fl(fl(sw * min(f_on, fl(f_oi - E2))) - E1o)          (object)
 *     LB_g = fl(fl(sw * f_g) - E1g),  LB_s = fl(fl(sw * f_sky) - E1s)
 * where f_* are the class-group minima of the segment (vB, vT) just evaluated: they are exact
 * integers that can only grow when the segment grows (class values >= 0 in FAST columns), the
 * terms left out are >= 0 (nic, pw / h) or >= -E (data terms, ic: PruneRec), and fp32 addition /
 * multiplication by a non-negative constant are monotone under round-to-nearest, so the bound
 * holds for the COMPUTED costs, not just the real-valued ones.  Once LB > best in every lane and
 * every type that can still receive candidates, the wave stops: nothing below can win, and nothing
 * below can tie (ties go to the smaller vB, hence the strict >). */
template <bool SKY, bool NOGROUND>
__device__ __forceinline__ bool nothing_below_can_win(const DevParams& P, const PruneVals& pv,
                                                      const SegTerms& t, const UnaryBest& b) {
    const float lb_o = P.sw * __builtin_fminf(t.f_on, t.f_oi - pv.E2) - pv.E1o;
    unsigned long long ok = __builtin_amdgcn_ballot_w64(lb_o > b.o) | pv.dead;
    if (SKY) {
        const float lb_s = P.sw * t.f_sky - pv.E1s;
        ok &= __builtin_amdgcn_ballot_w64(lb_s > b.s) | pv.dead;
    } else if (!NOGROUND) {
        const float lb_g = P.sw * t.f_g - pv.E1g;
        ok &= __builtin_amdgcn_ballot_w64(lb_g > b.g) | pv.gdead;
    }
    return ok == ~0ull;
}

/* steps vB, vB - nw, ... >= lower; returns the next vB, or INT_MIN once the wave is done */
#define IS_WAVE_DONE (-0x40000000)
template <bool HAS_INVALID, bool SKY, bool DIAG, bool PRUNE, int NR, bool NOGROUND>
__device__ __forceinline__ int unary_range_desc(const DevParams& P, const RowRec& my,
                                                const RowRec* __restrict__ rcol,
                                                const float* __restrict__ lcol, const float* my_tile,
                                                const float* s_rcp, int vT, int vTc, int vhor, int vB,
                                                int nw, int lower, bool row_ok, int lane4,
                                                __amdgpu_buffer_rsrc_t lrsrc, LutRow<NR>& next_row,
                                                const PruneVals& pv, UnaryBest& b) {
    float hf = (float)(vTc + 1 - vB);
    const float nwf = (float)nw;
    for (; vB >= lower; vB -= nw) {
        const RowRec cur = sload_rec(rcol + vB);
        const LutRow<NR> row = next_row;
        load_lut_row<NR>(next_row, lrsrc, lcol, max(vB - nw, 0), P.D, lane4);
        const SegTerms t = unary_step<true, HAS_INVALID, SKY, DIAG, false, NR, NOGROUND>(
            P, my, cur, row, my_tile, s_rcp, vT, vTc, vhor, vB, hf, row_ok, b);
        hf += nwf;
        if (PRUNE && nothing_below_can_win<SKY, NOGROUND>(P, pv, t, b)) return IS_WAVE_DONE;
    }
    return vB;
}

template <bool HAS_INVALID, int NR>
__device__ __forceinline__ void unary_loop_desc(const DevParams& P, const RowRec& my,
                                                const RowRec* __restrict__ rcol,
                                                const float* __restrict__ lcol, const float* my_tile,
                                                const float* s_rcp, int vT, int vTc, int vhor, int w,
                                                int nw, int tile_lo, int vB_end, int lane4,
                                                __amdgpu_buffer_rsrc_t lrsrc, const PruneRec* prec,
                                                UnaryBest& b) {
    const bool row_ok = vT < P.H;
    if (w > vB_end) return;
    int vB = vB_end - (vB_end - w) % nw; /* the wave's largest vB: vB == w (mod nw) */
    PruneVals pv = load_prune_vals(prec, 1.0f, row_ok);
    pv.gdead = pv.dead | __builtin_amdgcn_ballot_w64(my.G == IS_INF);
    LutRow<NR> next_row;
    load_lut_row<NR>(next_row, lrsrc, lcol, vB, P.D, lane4);
    const bool nog = tile_lo >= vhor;
#define IS_RANGE(SKY, DIAG, PRUNE, NOG, lower)                                                     \
    vB = unary_range_desc<HAS_INVALID, SKY, DIAG, PRUNE, NR, NOG>(P, my, rcol, lcol, my_tile, s_rcp,   \
                                                                  vT, vTc, vhor, vB, nw, lower, row_ok, \
                                                                  lane4, lrsrc, next_row, pv, b);  \
    if (vB == IS_WAVE_DONE) return
    /* (the horizon may lie outside the image: vhor < 0 or vhor >= H; vB = 0 is the FIRST step) */
    IS_RANGE(true, true, false, false, max(max(vhor, tile_lo) + 1, 1)); /* sky, diagonal block */
    IS_RANGE(true, false, true, false, max(vhor + 1, 1));               /* sky, whole wave live */
    IS_RANGE(false, true, false, false, max(tile_lo + 1, 1));   /* ground, diagonal block    */
    if (nog) {
        IS_RANGE(false, false, true, true, 1);                  /* ground candidates are +inf */
    } else {
        IS_RANGE(false, false, true, false, 1);
    }
#undef IS_RANGE
    if (vB == 0) { /* first segment (:481-594): ground + object */
        const RowRec cur = sload_rec(rcol);
        const LutRow<NR> row = next_row;
        if (tile_lo == 0)
            unary_step<true, HAS_INVALID, false, true, true, NR, false>(P, my, cur, row, my_tile, s_rcp, vT, vTc,
                                                                        vhor, 0, 0.0f, row_ok, b);
        else
            unary_step<true, HAS_INVALID, false, false, true, NR, false>(P, my, cur, row, my_tile, s_rcp, vT, vTc,
                                                                         vhor, 0, 0.0f, row_ok, b);
    }
}

/* FASTCOLS: the launch handles only the columns of that encoding (col_flags), workgroups of the
 * other kind leave at once.  Two lean kernels instead of one that carries both loop nests: no
 * register spills, and the generic launch costs ~nothing when every column is FAST. */
/* GATED (FASTCOLS only): the repair launch behind k_unary_path (is_k_unary_path.hip), which leaves at once while
 * the word `n_generic` points to -- the path's distrust word then -- is 0, like the generic launch. */
template <bool HAS_INVALID, int NR, bool FASTCOLS, bool GATED = false>
__global__ __launch_bounds__(IS_UNARY_WAVES * 64, IS_UNARY_OCC) void k_dp_unary(const DevParams P, int ncols,
                                                  const RowRec* __restrict__ recs,
                                                  const float* __restrict__ lutT,
                                                  const float* __restrict__ rcp,
                                                  const int* __restrict__ vhor_arr,
                                                  const int* __restrict__ col_flags,
                                                  const PruneRec* __restrict__ prune,
                                                  float* __restrict__ cost_table,
                                                  int32_t* __restrict__ index_table,
                                                  const int* __restrict__ n_generic,
                                                  int pairs_per_wg) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int H = P.H, D = P.D;
    const int DP = D + 1; /* padded row: conflict-free when lanes share fni */
    float* s_rcp = (float*)smem;              /* [H+1 -> x4] RN(1/h), kept across both tiles   */
    float* s_tile = s_rcp + ((H + 1 + 3) & ~3); /* [64][D+1] lutT rows tile_lo+1 .. tile_lo+64  */

    /* XCD-aware order: blocks b, b+8, ... share an XCD/L2; keep all tiles of a column on one
     * XCD (they gather from the same lutT) and start with the tallest tiles. */
    const int nxcd = 8;
    const int npairs = (P.ntiles + 1) / 2;
    const int wg_per_col = (npairs + pairs_per_wg - 1) / pairs_per_wg;
    /* The launch of the generic columns is a small grid that walks all (column, tile pair) items
     * and leaves at once when the batch has no generic column (k_prepare_columns counts them):
     * a full grid of workgroups that each only read their column's flag cost 0.13 ms per 64
     * frames in dispatch alone. */
    if ((!FASTCOLS || GATED) && __builtin_amdgcn_readfirstlane(*n_generic) == 0) return;
    const int n_items = ((ncols + nxcd - 1) / nxcd) * nxcd * wg_per_col;
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
    __syncthreads(); /* the previous item's merge area aliases this item's LUT tile */
    /* (integer division runs on the VALU: pin the uniform results back into SGPRs) */
    const int xcd = item % nxcd, q = item / nxcd;
    const int wg_in_col = __builtin_amdgcn_readfirstlane(q % wg_per_col);
    const int colg = __builtin_amdgcn_readfirstlane((q / wg_per_col) * nxcd + xcd);
    if (colg >= ncols) continue;
    if ((__builtin_amdgcn_readfirstlane(col_flags[colg]) == 0) != FASTCOLS) continue;
    const int img = __builtin_amdgcn_readfirstlane(colg / P.C);
    const int vhor = __builtin_amdgcn_readfirstlane(vhor_arr[img]);

    const int tid = threadIdx.x, lane = tid & 63;
    const int nw = blockDim.x >> 6;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const RowRec* rcol = recs + (size_t)colg * (H + 1);
    const float* lcol = lutT + (size_t)colg * (H + 1) * D;
    stage_rcp(s_rcp, rcp, H, tid, (int)blockDim.x);
    const __amdgpu_buffer_rsrc_t lrsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void*)lcol, 0, (H + 1) * D * (int)sizeof(float), 0x00020000 /* raw, 32-bit data */);

    /* a workgroup takes the tile pair (ntiles-1-pair, pair): every workgroup then carries the
     * same number of (vB, vT) pairs, and the per-workgroup fixed costs are paid half as often */
    bool first = true;
    for (int pair = wg_in_col; pair < npairs; pair += wg_per_col) {
    const int n_pass = (P.ntiles - 1 - pair == pair) ? 1 : 2;
    for (int pass = 0; pass < n_pass; pass++) {
    const int tile = pass == 0 ? (P.ntiles - 1 - pair) : pair;
    const int tile_lo = tile * IS_TILE;
    if (!first) __syncthreads(); /* the merge area of the previous tile aliases the LUT tile */
    first = false;

    stage_lut_tile<false>(s_tile, lcol, tile_lo, H, D, tid, (int)blockDim.x);

    const int vT = tile_lo + lane;
    const int vTc = min(vT, H - 1);
    const RowRec my = load_rec(rcol + vTc + 1);
    __syncthreads();

    UnaryBest b;
    unary_best_init(b);
    const float* my_tile = s_tile + lane * DP;
    const int vB_end = min(tile_lo + IS_TILE - 1, H - 1);
    if (FASTCOLS)
        unary_loop_desc<HAS_INVALID, NR>(P, my, rcol, lcol, my_tile, s_rcp, vT, vTc, vhor, w, nw, tile_lo,
                                         vB_end, lane * 4, lrsrc, prune + colg, b);
    else
        unary_loop<HAS_INVALID, NR>(P, my, rcol, lcol, my_tile, s_rcp, vT, vTc, vhor, w, nw, tile_lo, vB_end,
                                    lane * 4, lrsrc, b);

    /* merge the waves' partial minima and store the tile's rows (the merge area aliases the LUT tile, the finals
     * wave 0's slot of it) */
    UNARY_MERGE_STORE(s_tile, s_tile, b, nw, w, tid, lane, colg, H, vT, cost_table, index_table);
    } /* pass */
    } /* pair */
    } /* item */
}

/* The instantiation for (invalid-disparity value or none, D <= 128, form): the only ones the library holds.
 * D <= 128: the vB-side lutT row travels in two registers per lane (LutRow<2>); wider tables gather per lane. */
enum { IS_UNARY_FASTCOLS = 0, IS_UNARY_GENERIC = 1, IS_UNARY_REPAIR = 2, IS_UNARY_FORMS = 3 };
using UnaryKernel = decltype(&k_dp_unary<false, 2, true>);
template <bool INV, int NR>
static UnaryKernel unary_kernel_form(int form) {
    const UnaryKernel k[IS_UNARY_FORMS] = {k_dp_unary<INV, NR, true>, k_dp_unary<INV, NR, false>,
                                           k_dp_unary<INV, NR, true, true>}; /* [IS_UNARY_*] */
    return form >= 0 && form < IS_UNARY_FORMS ? k[form] : nullptr;
}
static UnaryKernel unary_kernel(bool invalid, bool d128, int form) {
    if (d128) return invalid ? unary_kernel_form<true, 2>(form) : unary_kernel_form<false, 2>(form);
    return invalid ? unary_kernel_form<true, 0>(form) : unary_kernel_form<false, 0>(form);
}

extern "C" {

size_t isk_unary_lds_bytes(const DevParams* P) {
    const size_t rcp = sizeof(float) * (((size_t)P->H + 1 + 3) & ~(size_t)3);
    const size_t tile = sizeof(float) * (size_t)IS_TILE * (P->D + 1);
    /* (aliases the tile after the loop) */
    const size_t merge = sizeof(float) * UNARY_MERGE_FLOATS((size_t)IS_UNARY_WAVES);
    return rcp + (tile > merge ? tile : merge) + 16;
}

/* The unary DP of a call, as plan_call decided:
 *  - the walk (is_k_unary_path.hip): the visited rows of the FAST columns, then the generic columns in full (leaves at
 *    once when the call has none), then the repair: the tile-path DP of every FAST column again, leaving at once
 *    while k_unary_path has not set path_bad.  The prepare launch stored only the LUT's block carries (lutC), so each
 *    of the two is preceded by a gated launch that builds the complete lutT of the columns it takes
 *    (isk_launch_lut_generic: the generic columns; isk_launch_lut_repair on path_bad: every column);
 *  - the tile path: the FAST columns through k_dp_unary_fast (plan->unary_nvr) or the kernel of this file, then the
 *    generic columns. */
hipError_t isk_launch_dp_unary(const DevParams* P, const CallPlan* plan, const CallBuffers* b, hipStream_t stream) {
    const int ncols = plan->ncols;
    hipError_t e = hipSuccess;
    if (plan->unary_walk)
        e = isk_launch_unary_path(P, plan, b, stream);
    else if (plan->unary_nvr)
        e = isk_launch_dp_unary_fast(P, plan, b, stream);
    if (e != hipSuccess) return e;
    /* one tile pair (big, small) per workgroup: equal-length workgroups pack best; measured on
     * MI355X at batch 32: 1 pair 9.98 ms, 2 pairs 10.10 ms, 4 pairs 10.55 ms, single tiles 11.1 ms */
    const int npairs = (P->ntiles + 1) / 2;
    const int pairs_per_wg = 1;
    const unsigned items = (unsigned)((ncols + 7) / 8) * 8u * (unsigned)npairs;
    const dim3 grid_generic(items < 16384u ? items : 16384u); /* walks the items, see the kernel */
    const dim3 grid_repair(items < 2048u ? items : 2048u);    /* (walks the items: a safety net, not a fast path) */
    const bool inv = P->invalid >= 0, d128 = P->D <= 128;
    auto launch = [&](int form, dim3 grid, const int* gate) {
        const UnaryKernel k = unary_kernel(inv, d128, form);
        if (k == nullptr) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k, grid, dim3(plan->nwaves * 64), isk_unary_lds_bytes(P), stream, *P, ncols, b->recs, b->lutT,
                           b->rcp, b->vhor, b->col_flags, b->prune, b->cost_table, b->index_table, gate, pairs_per_wg);
        return hipSuccess;
    };
    if (!plan->unary_walk && !plan->unary_nvr) e = launch(IS_UNARY_FASTCOLS, dim3(items), b->n_generic);
    if (e == hipSuccess && plan->lut_carry) e = isk_launch_lut_generic(P, plan, b, stream);
    if (e == hipSuccess) e = launch(IS_UNARY_GENERIC, grid_generic, b->n_generic);
    if (e == hipSuccess && plan->unary_walk) {
        if (plan->lut_carry) e = isk_launch_lut_repair(P, ncols, b->joined, b->cost_T, b->lutT, b->path_bad, stream);
        if (e == hipSuccess) e = launch(IS_UNARY_REPAIR, grid_repair, b->path_bad);
    }
    return e != hipSuccess ? e : hipGetLastError();
}

int isk_debug_occupancy(const DevParams* P, int nwaves) {
    int nb = -1;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)unary_kernel(false, true, IS_UNARY_FASTCOLS),
                                                       nwaves * 64, isk_unary_lds_bytes(P));
    return nb;
}

/* (the instantiations this context's D and invalid value can launch) */
hipError_t isk_set_lds_unary(const DevParams* P) {
    hipError_t e = hipSuccess;
    for (int form = 0; form < IS_UNARY_FORMS && e == hipSuccess; form++)
        e = hipFuncSetAttribute((const void*)unary_kernel(P->invalid >= 0, P->D <= 128, form),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)isk_unary_lds_bytes(P));
    return e != hipSuccess ? e : isk_set_lds_unary_fast(P);
}

} /* extern "C" */
