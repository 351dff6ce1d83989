/*
 * is_unary.h -- what the three kernels of the unary column DP share: k_dp_unary (tile pairs, is_k_unary.hip),
 * k_dp_unary_fast (ring and windows, is_k_unary_fast.hip) and k_unary_path (the walk, is_k_unary_path.hip) evaluate
 * the same segment (vB, vT) by the same rules.  How a kernel obtains the segment's terms, its object data term and
 * 1/h is its own (scalar record + pick_lut, ring slot + window, LDS quarters, rebuilt LUT entries), and so are its
 * bounds; the cost, the update of the bests, the merge and the final index exist here, once.
 */
#ifndef IS_UNARY_H_
#define IS_UNARY_H_

#include "is_kernels.h"

/* In unary mode the predecessor cost is never added: cost_table[vT][t] is the
 * minimum over vB of a single-segment cost, so all (vB, vT) pairs are independent and the only
 * order that matters is the strict-< tie rule (smallest vB wins).  index_table holds the winning
 * vB (or -1); the predecessor TYPE is resolved in k_backtrace from the final cost_table. */
struct UnaryBest {
    float g, o, s;
    int vg, vo, vs;
};
__device__ __forceinline__ void unary_best_init(UnaryBest& b) {
    b.g = b.o = b.s = IS_INF;
    b.vg = b.vs = -1;
    b.vo = 0; /* index_table[vT*3+OBJECT] = OBJECT at vB = 0, :592 */
}

/* register copy of a PruneRec + the lanes that need no bound.  e2_factor: 1 for nothing_below_can_win (class
 * minima), 3 for fast_bounds (seg_o_lower_bound, is_kernels.h).  gdead starts as dead: the caller completes it with
 * ballot(my.G == IS_INF) once the lane's record is here. */
struct PruneVals {
    float E1o, E1g, E1s, E2;
    unsigned long long dead;  /* lanes with vT >= H: never stored                         */
    unsigned long long gdead; /* dead, or the ground data term of the lane is +inf for good */
};
__device__ __forceinline__ PruneVals load_prune_vals(const PruneRec* prec, const float e2_factor, const bool row_ok) {
    cprune_t q = (cprune_t)prec;
    PruneVals pv;
    pv.E1o = q->E1o; pv.E1g = q->E1g; pv.E1s = q->E1s;
    pv.E2 = e2_factor * q->E2; /* (x * 1.0f is x) */
    pv.dead = ~__builtin_amdgcn_ballot_w64(row_ok);
    pv.gdead = pv.dead;
    return pv;
}

/* cost = dw*data + pw*(1/h) + sw*seg, left to right (StixelsKernels.cu:716-719, 762-765, 820-823); pwih = pw * RN(1/h).
 * The build has -ffp-contract=off: two multiplications and two additions, each rounded, never an FMA. */
__device__ __forceinline__ float unary_cost(const DevParams& P, const float data, const float pwih, const float seg) {
    return P.dw * data + pwih + P.sw * seg;
}

/* The update of the three bests by one (vB, vT) evaluation: the object candidate, then
 *   SKY      the sky candidate: the segment's lower neighbour is at / above the horizon (vB-1 >= vhor, :729);
 *            otherwise the GROUND candidate (:687); wave-uniform, so the callers run separate loops / branches and
 *            each has ONE accumulator pair live in its body;
 *   NOGROUND neither: every lane of the tile lies at or above the horizon, where the ground data cost prefix is
 *            +inf (StixelsKernels.cu:435-446): dw * inf is inf (or NaN for dw = 0) and never wins, so the candidate
 *            is not evaluated at all;
 *   DIAG     the segment start may lie above this lane's vT (diagonal 64x64 block): masked lanes (`live`);
 *   FIRST    vB = 0: ground additionally needs vT <= vhor (:542-545; `below_hor`, read by FIRST steps only);
 *   LE       the `<=` of a DESCENDING walk over vB (among equal costs the smallest vB must win, as in the reference's
 *            ascending loop, whose strict `<` is the form without LE).  A +inf candidate passes `<=` against the
 *            initial +inf: unary_final_index restores the initial index.
 * Full steps of a descending walk (LE, neither DIAG nor FIRST): every lane with vT < H is live and rows vT >= H are
 * never stored, so they take take_if_le (vB wave-uniform there); all others a masked select. */
template <bool LE, bool SKY, bool DIAG, bool FIRST, bool NOGROUND>
__device__ __forceinline__ void unary_update(const DevParams& P, const SegTerms& t, const float od, const float pwih,
                                             const int vB, const bool live, const bool below_hor, UnaryBest& b) {
    constexpr bool ALL_LANES = LE && !DIAG && !FIRST;
    const float cost_o = unary_cost(P, od, pwih, t.seg_o);
    if constexpr (ALL_LANES) {
        take_if_le(b.o, b.vo, cost_o, vB);
    } else {
        const bool uo = live && (LE ? (cost_o <= b.o) : (cost_o < b.o));
        b.o = uo ? cost_o : b.o;
        b.vo = uo ? vB : b.vo;
    }
    if constexpr (SKY) {
        const float cost_s = unary_cost(P, t.sd, pwih, t.seg_s);
        if constexpr (ALL_LANES) {
            take_if_le(b.s, b.vs, cost_s, vB);
        } else {
            const bool us = live && (LE ? (cost_s <= b.s) : (cost_s < b.s));
            b.s = us ? cost_s : b.s;
            b.vs = us ? vB : b.vs;
        }
    } else if constexpr (!NOGROUND) {
        const float cost_g = unary_cost(P, t.gd, pwih, t.seg_g);
        if constexpr (ALL_LANES) {
            take_if_le(b.g, b.vg, cost_g, vB);
        } else {
            const bool ug = (FIRST ? (live && below_hor) : live) && (LE ? (cost_g <= b.g) : (cost_g < b.g));
            b.g = ug ? cost_g : b.g;
            b.vg = ug ? vB : b.vg;
        }
    }
}

/* The merge of partial minima of one row and type -- of the waves of a tile kernel, of the quarters of a diagonal
 * block, of the lanes of the walk: min cost, ties -> the smallest recorded vB (= the first strict minimum of the
 * reference's ascending-vB loop; a partial minimum without a candidate has v < 0 and never wins a tie).
 * The walk evaluates the same rule over its 64 lanes as a reduction (unary_merge_lanes, is_k_unary_path.hip). */
/* (a macro under the function: with the rule in a function of its own under unary_merge_take, k_unary_path compiled to
 * other code than before and its call measured 1.4 % slower) */
#define UNARY_MERGE_WINS(c, v, c2, v2) (((c2) < (c)) || ((c2) == (c) && (v2) >= 0 && ((v) < 0 || (v2) < (v))))
__device__ __forceinline__ void unary_merge_take(float& c, int& v, float c2, int v2) {
    const bool take = UNARY_MERGE_WINS(c, v, c2, v2);
    c = take ? c2 : c;
    v = take ? v2 : v;
}
/* a row without a finite candidate keeps the initial index (the descending walks record +inf candidates, the
 * reference's strict < never does; :592 for the object type) */
__device__ __forceinline__ int unary_final_index(const int type, const float c, const int v) {
    return !(c < IS_INF) ? ((type == IS_OBJECT) ? 0 : -1) : v;
}

/* The waves' partial minima of a tile merged and the tile's rows stored, with their three barriers.  s_merge: a slot
 * per wave, [3][64] costs, then [3][64] indices (UNARY_MERGE_FLOATS), in the space of the tile's lutT rows -- behind
 * the first barrier no wave reads the tile any more.  Wave `type` merges that type and leaves the final (cost, vB) in
 * s_final, one more slot: one wave then writes the three types of a row as 12 contiguous bytes (a wave-wide contiguous
 * 768-byte store) instead of three waves writing every third dword.  s_final may be s_merge itself, wave 0's slot (a
 * thread has read its own entry of that slot before it writes it).  Rows vT >= H are not stored.
 * A macro, and the place of the finals left to the caller, because of the register allocator. */
#define UNARY_SLOT_FLOATS (3 * 64 * 2)
#define UNARY_MERGE_FLOATS(nw) ((nw) * UNARY_SLOT_FLOATS)
#define UNARY_MERGE_STORE(s_merge, s_final, b, nw, w, tid, lane, colg, H, vT, cost_table, index_table)               \
    do {                                                                                                             \
        __syncthreads();                                                                                             \
        float* m_cost_ = (s_merge);                                                                                  \
        int* m_vb_ = (int*)(m_cost_ + 3 * 64);                                                                       \
        float* f_cost_ = (s_final);                                                                                  \
        int* f_vb_ = (int*)(f_cost_ + 3 * 64);                                                                       \
        m_cost_[((w) * 6 + 0) * 64 + (lane)] = (b).g; m_vb_[((w) * 6 + 0) * 64 + (lane)] = (b).vg;                   \
        m_cost_[((w) * 6 + 1) * 64 + (lane)] = (b).o; m_vb_[((w) * 6 + 1) * 64 + (lane)] = (b).vo;                   \
        m_cost_[((w) * 6 + 2) * 64 + (lane)] = (b).s; m_vb_[((w) * 6 + 2) * 64 + (lane)] = (b).vs;                   \
        __syncthreads();                                                                                             \
        if ((tid) < 3 * 64) {                                                                                        \
            const int type_ = (tid) >> 6;                                                                            \
            float c_ = m_cost_[(0 * 6 + type_) * 64 + (lane)];                                                       \
            int vb_ = m_vb_[(0 * 6 + type_) * 64 + (lane)];                                                          \
            for (int ww_ = 1; ww_ < (nw); ww_++)                                                                     \
                unary_merge_take(c_, vb_, m_cost_[(ww_ * 6 + type_) * 64 + (lane)],                                  \
                                 m_vb_[(ww_ * 6 + type_) * 64 + (lane)]);                                            \
            f_cost_[type_ * 64 + (lane)] = c_;                                                                       \
            f_vb_[type_ * 64 + (lane)] = unary_final_index(type_, c_, vb_);                                          \
        }                                                                                                            \
        __syncthreads();                                                                                             \
        if ((w) == 0 && (vT) < (H)) {                                                                                \
            const size_t o_ = ((size_t)(colg) * (H) + (vT)) * 3;                                                     \
            float* cd_ = (cost_table) + o_;                                                                          \
            int32_t* id_ = (index_table) + o_;                                                                       \
            cd_[0] = f_cost_[0 * 64 + (lane)]; cd_[1] = f_cost_[1 * 64 + (lane)]; cd_[2] = f_cost_[2 * 64 + (lane)]; \
            id_[0] = f_vb_[0 * 64 + (lane)]; id_[1] = f_vb_[1 * 64 + (lane)]; id_[2] = f_vb_[2 * 64 + (lane)];       \
        }                                                                                                            \
    } while (0)

#endif /* IS_UNARY_H_ */
