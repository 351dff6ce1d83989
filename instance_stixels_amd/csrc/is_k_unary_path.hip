/* is_k_unary_path.hip -- the unary DP along the back-trace's own path.  See is_kernels.h. */
#include "is_unary.h"

/* ====================================================================================== */
/* Unary DP of the visited rows only: one wave per column                                  */
/* ====================================================================================== */
/* In unary mode the predecessor cost is never added, so row vT of the tables (min / arg-min over vB of one
 * segment's cost, per type) depends on no other row, and k_backtrace reads only the rows on its path: row
 * H - 1, then row vB - 1 of every Section it emits.  This kernel walks that path itself: it computes a row
 * completely, picks the type with k_backtrace's rules, takes vB from the index of that type and goes on at
 * vT = vB - 1.  It writes the three (cost, index) pairs of every visited row at their usual addresses and
 * leaves every other row alone; the unchanged k_backtrace behind it then reads exactly those rows.
 *
 * A row: the lanes are 64 consecutive candidates vB = 64 s + 1 + lane, walked downwards in s, then the first
 * segment vB = 0 in lane 0.  Each candidate is the tile path's evaluation (eval_segment with my = record vT + 1,
 * rb = record vB, the cost assembly of unary_step) with the per-lane cases of the tile kernels: SKY when
 * vB - 1 >= vhor, otherwise GROUND; FIRST (vB = 0): ground only when vT <= vhor.  A lane's candidates descend,
 * so it keeps the LAST of equal costs (<=, take_if_le's rule); the lanes merge by the tile path's rule
 * (min cost, ties -> smallest vB, +inf -> the initial index), evaluated as two DPP minima per type on the VALU
 * (unary_merge_lanes); the row's six numbers come out as scalars.  NaN candidates never pass <=.
 *
 * Pruning (lemma L5): the class-group minima f_* of the LONGEST segment of a step (lane 0,
 * vB = 64 s + 1) bound the cost of every candidate vB' <= vB of the row, per type.  A type whose bound exceeds
 * the row's best so far (some lane's best < lb) closes for the rest of the row; the row ends when every type
 * that can still receive candidates is closed.  A column whose E1o is +inf (IS_NO_PRUNE, non-finite
 * weights) is walked in full.
 *
 * The object table: the prepare launch of a walk call stores only its block carries lutC[k][fn] =
 * lutT[32 k][fn] (CallPlan::lut_carry).  The lanes of a step are exactly LUT blocks 2 s and 2 s + 1 (lane l: candidate
 * vB = 64 s + 1 + l, entry lutT[64 s + l + 1] = output l & 31 of block 2 s + l / 32), so the wave rebuilds the entries
 * of a step with the reference's own 32-lane network, lanes = rows, once per distinct fn of the step (lut_network).
 * The vT side, lutT[vT + 1][fn], is output vT & 31 of block vT / 32: picked from the first step's networks when that
 * block is among them, otherwise built two fn at a time (lut_row_entry), and kept per row in an LDS cache.
 *
 * The held block: rows descend, and most hops start the next row in the 64-row block whose
 * records the wave loaded last, so path_row keeps the records of its last full step in the lanes across rows and a
 * step on that block loads nothing; record vT + 1 is then the previous hop's vB and comes from the lane that owns it.
 *
 * Sections (CallPlan::walk_sections, a call without instance outputs): lane 0 records (vT, vB, type, cost) of every
 * hop in LDS; after a chain that succeeded the lanes build the Sections with k_backtrace's make_section and store them
 * with the terminator, and k_backtrace runs gated (generic columns, every column of a distrusted call).
 *
 * What the kernel cannot reproduce it does not try to: a chosen index outside [0, vT] (every candidate of
 * the type +inf or NaN) sets *bad, and the repair launches behind this one redo the whole call on the tile
 * path.  Generic-encoding columns (col_flags != 0) are left to k_dp_unary<.., false>, as on the tile path. */
/* One column's object table as the walk reads it: the carries, the disparities, the fn-major cost table and the
 * LDS cache of row vT + 1 (s_tag[fn] = the row whose entry s_val[fn] holds) */
struct LutCol {
    const float* __restrict__ dcol;  /* [H] joined disparities */
    const float* __restrict__ ccol;  /* [nb][D] lutC: lutT[32 k] */
    const float* __restrict__ costF; /* [fn][dis] */
    int* s_tag;
    float* s_val;
    int* s_my; /* [32]: spread_of_lane */
    int H, D, nb;
};

/* Half h of the wave (lanes 32 h .. 32 h + 31) runs LUT block blk of fn (both per half): lane 32 h + p returns
 * lutT[32 blk + p + 1][fn].  object_lut_body's network with lanes = rows -- the reference's own layout
 * (StixelsKernels.cu:249-266): c = obj_cost_lut[fn][dis of row 32 blk + p], lane 0 of the half first adds the carry
 * (c[0] += add, block 0 included), then c[p] += c[p - j] for j = 1, 2, 4, 8, 16 within the half.  The same
 * additions on the same values: the same bits. */
__device__ __forceinline__ float lut_network(const LutCol& L, int dis, int fn, int blk, int lane) {
    asm volatile("" : "+v"(lane)); /* (the shuffle indices and the p >= j masks are rebuilt here, not kept per kernel) */
    const int p = lane & 31;
    float c = L.costF[(size_t)fn * L.D + dis];
    if (p == 0) c += L.ccol[(size_t)blk * L.D + fn];
#pragma unroll
    for (int j = 1; j < 32; j <<= 1) {
        /* lane - j (mod 64): only p >= j takes it, and there it is __shfl_up(c, j, 32) */
        const float t = __int_as_float(__builtin_amdgcn_ds_bpermute(4 * lane + 4 * (64 - j), __float_as_int(c)));
        if (p >= j) c += t;
    }
    return c;
}

/* A record whose address is the same in every lane, held in ONE VGPR: lane i (and i + 32) has dword i.  The fields
 * come out with v_readlane (SGPR operands of the evaluation), so the record costs one VGPR instead of 32. */
__device__ __forceinline__ int load_rec_spread(const RowRec* p, int lane) {
    asm volatile("" : "+v"(lane)); /* (the address is rebuilt at the load, not kept in two VGPRs for the kernel) */
    return ((const int*)p)[lane & 31];
}
__device__ __forceinline__ RowRec rec_of_spread(int v) {
    RowRec r;
    int* d = (int*)&r;
#pragma unroll
    for (int i = 0; i < 32; i++) d[i] = __builtin_amdgcn_readlane(v, i);
    return r;
}
/* ... and the record that lane l of a block of records (one per lane) holds, in that form: through 128 bytes of
 * LDS (eight 16-byte writes of one lane, one read), about a tenth of the latency of the load it replaces */
__device__ __forceinline__ int spread_of_lane(const RowRec& blk, int l, int lane, int* s_my) {
    if (lane == l) {
#pragma unroll
        for (int i = 0; i < 8; i++) ((int4*)s_my)[i] = ((const int4*)&blk)[i];
    }
    __syncthreads(); /* (one wave) */
    int v = s_my[lane & 31];
    asm volatile("" : "+v"(v)); /* (an LDS read: not merged with the miss's global load into one flat load) */
    return v;
}

/* lutT[vT + 1][fni] for the lanes in `need` (others: 0).  Cache misses are built two fn per pass, one per half,
 * with the network of block vT / 32; disT: the bin of row 32 (vT / 32) + (lane & 31). */
__device__ __forceinline__ float lut_row_entry(const LutCol& L, int disT, int vT, int fni, bool need, int lane) {
    const int tag = vT + 1, kT = vT >> 5, pT = vT & 31;
    __syncthreads(); /* (one wave) the cache writes above before its reads */
    float v = 0.0f;
    bool miss = false;
    if (need) {
        miss = L.s_tag[fni] != tag;
        v = L.s_val[fni];
    }
    uint64_t m = __builtin_amdgcn_ballot_w64(miss);
    while (m != 0ull) {
        const int fa = __builtin_amdgcn_readlane(fni, __builtin_ctzll(m));
        m &= ~__builtin_amdgcn_ballot_w64(fni == fa);
        const int fb = m != 0ull ? __builtin_amdgcn_readlane(fni, __builtin_ctzll(m)) : fa;
        m &= ~__builtin_amdgcn_ballot_w64(fni == fb);
        const float out = lut_network(L, disT, lane < 32 ? fa : fb, kT, lane);
        const float va = readlane_f(out, pT), vb = readlane_f(out, 32 + pT);
        v = fni == fa ? va : (fni == fb ? vb : v);
        if (lane == 0) {
            L.s_tag[fa] = tag; L.s_val[fa] = va;
            L.s_tag[fb] = tag; L.s_val[fb] = vb;
        }
    }
    return v;
}

/* The lanes' partial minima of a row merged: unary_merge_take's rule (is_unary.h) evaluated as a reduction, all on
 * the VALU -- no LDS round trip, no wait, no branch.  Per type two wave-wide minima by DPP (row_shr:1/2/4/8 leave a
 * row's minimum in its lane 15, row_bcast:15 / row_bcast:31 carry it on: lane 63 holds the wave's), each read with
 * v_readlane:
 *   m    = min of c (a best is never NaN);
 *   vmin = the smallest recorded vB among the lanes with c == m, as an unsigned minimum of a key: v where c == m,
 *          -1 = 0xFFFFFFFF in the lanes that lost -- and a lane that recorded nothing has v = -1, the same key, of
 *          itself; recorded vB of different lanes differ;
 *   the cost that goes on: the bits of the one lane whose key is vmin (equal-comparing costs, -0 / +0, take the bits
 *          of the smaller vB, as a butterfly of takes does).  When no lane has a key, the lanes at the minimum hold
 *          the initial pair, m is +inf and so is every lane's cost: vmin = -1 matches them all and any lane's bits do.
 * The results are wave-uniform: scalars. */
/* (one statement for the three types: between the write of a register and its next DPP read stand the two other
 * types' instructions, the two wait states that read needs; the compiler does not look inside, so the s_nop in front
 * -- five wait states: a VALU write of the registers (two) or of EXEC (five) may stand right before the statement --
 * travels with it.  dst = src: a lane
 * without a source or outside the row mask is not written and keeps its own value, bound_ctrl off.) */
#define IS_WAVE_MIN3(OP)                                                                                             \
    asm("s_nop 4\n\t"                                                                                                \
        IS_WAVE_MIN3_STEP(OP, "row_shr:1 row_mask:0xf") IS_WAVE_MIN3_STEP(OP, "row_shr:2 row_mask:0xf")              \
        IS_WAVE_MIN3_STEP(OP, "row_shr:4 row_mask:0xf") IS_WAVE_MIN3_STEP(OP, "row_shr:8 row_mask:0xf")              \
        IS_WAVE_MIN3_STEP(OP, "row_bcast:15 row_mask:0xa") IS_WAVE_MIN3_STEP(OP, "row_bcast:31 row_mask:0xc")        \
        : "+v"(a), "+v"(b), "+v"(c))
#define IS_WAVE_MIN3_STEP(OP, CTRL)                                                                                  \
    OP " %0, %0, %0 " CTRL " bank_mask:0xf\n\t" OP " %1, %1, %1 " CTRL " bank_mask:0xf\n\t"                          \
    OP " %2, %2, %2 " CTRL " bank_mask:0xf\n\t"
/* lane 63 of a, b, c: their minima over the wave (floats: no NaN among them) */
__device__ __forceinline__ void wave_min3_f(float& a, float& b, float& c) { IS_WAVE_MIN3("v_min_f32_dpp"); }
__device__ __forceinline__ void wave_min3_u(unsigned& a, unsigned& b, unsigned& c) { IS_WAVE_MIN3("v_min_u32_dpp"); }
#undef IS_WAVE_MIN3_STEP
#undef IS_WAVE_MIN3

struct PathBest {
    float c[3];
    int v[3];
};

/* c / v: the lanes' (cost, vB) pairs in the order of the types (IS_GROUND, IS_OBJECT, IS_SKY) */
__device__ __forceinline__ PathBest unary_merge_lanes(const float (&c)[3], const int (&v)[3]) {
    float m[3] = {c[0], c[1], c[2]};
    wave_min3_f(m[0], m[1], m[2]);
    unsigned key[3], k[3];
#pragma unroll
    for (int t = 0; t < 3; t++) {
        key[t] = c[t] == readlane_f(m[t], 63) ? (unsigned)v[t] : 0xFFFFFFFFu; /* (v = -1: no key as it stands) */
        k[t] = key[t];
    }
    wave_min3_u(k[0], k[1], k[2]);
    PathBest b;
#pragma unroll
    for (int t = 0; t < 3; t++) {
        /* (no lane qualifies: vmin = -1 matches every lane, and every lane's cost is m = +inf) */
        const unsigned vmin = (unsigned)__builtin_amdgcn_readlane((int)k[t], 63);
        const uint64_t own = __builtin_amdgcn_ballot_w64(key[t] == vmin);
        b.c[t] = readlane_f(c[t], __builtin_ctzll(own));
        b.v[t] = unary_final_index(t, b.c[t], (int)vmin);
    }
    return b;
}

template <bool HAS_INVALID>
__device__ __forceinline__ PathBest path_row(const DevParams& P, const RowRec* __restrict__ rcol, const LutCol& L,
                                             const float* __restrict__ rcp, const PruneRec& pr, int vT, int vhor,
                                             int lane, int& cs, RowRec& cb) {
    const int D = P.D;
    /* The block of the last full step stays in the lanes across rows (cs: its index s, cb: the record of candidate
     * 64 cs + 1 + lane).  Rows descend, so a lane that is live in a later row of the same block (vB <= vT) was live
     * when the block was loaded and holds its own record; the dead lanes (vB > vT) hold their own record or the
     * clamped one of the loading row (a row >= vT + 1 of this column): every index derived from them is clamped --
     * h = vT + 1 - vBc = 1 (rcp[1]), the valid count through cvt_u32_sat into rcp[0 .. H] (V differences are in
     * [-H, H]), fni into [0, D - 1] -- and nothing of them passes `live`.
     * Record vT + 1 (`my`) is one VGPR for the wave (load_rec_spread): 32 VGPRs go to the block instead.  When the
     * row starts in the held block and vT + 1 is one of its candidates (the previous hop's vB, lane vT - 64 cs), the
     * owning lane hands it over; otherwise (a miss, or vT = 64 s + 64: vT + 1 belongs to the block above) one
     * 128-byte load. */
    int myv;
    {
        const int s0 = (vT - 1) >> 6, l0 = vT - 64 * s0;
        if (s0 >= 0 && s0 == cs && l0 < 64) myv = spread_of_lane(cb, l0, lane, L.s_my);
        else myv = load_rec_spread(rcol + vT + 1, lane);
    }
#define IS_MY_REC() asm volatile("" : "+v"(myv)); const RowRec my = rec_of_spread(myv) /* (not hoisted: SGPRs) */
    const float myG = __int_as_float(__builtin_amdgcn_readlane(myv, offsetof(RowRec, G) / 4));
    const int disT = lut_bin(lut_row_d(L.dcol, (vT & ~31) + (lane & 31), L.H), D);
    const int s_first = (vT - 1) >> 6;
    float bg = IS_INF, bo = IS_INF, bs = IS_INF;
    int vg = -1, vo = -1, vs = -1;
    const bool prune_on = pr.E1o < IS_INF;
    bool open_o = true, open_s = true;
    /* ground data cost +inf from this row on (at / above the horizon): no ground candidate can win */
    bool open_g = !(myG == IS_INF);
    /* Full steps while the object type is open, then ground- / sky-only steps: the close is monotone within a row.
     * `ended`: the exit test fired, nothing below can win (the first segment included). */
    bool ended = false;
    int s = s_first; /* (vT = 0: -1, no candidate vB >= 1) */
    for (; s >= 0 && open_o; s--) {
        const int vB = 64 * s + 1 + lane;
        const bool live = vB <= vT;
        const int vBc = live ? vB : vT;
        IS_MY_REC();
        if (s != cs) { cb = load_rec(rcol + vBc); cs = s; }
        const RowRec& rb = cb;
        const int disS = lut_bin(lut_row_d(L.dcol, 64 * s + lane, L.H), D); /* rows of the step's two LUT blocks */
        const int h = vT + 1 - vBc;
        const float r = rcp[h]; /* RN(1/h) */
        const SegTerms t = eval_segment<true, HAS_INVALID>(my, rb, (float)h, r, D, P.iw, rcp);
        const float pwih = P.pw * r;
        /* (ground and sky, and everything of the bounds but the object type's ballot, in front of the networks:
         * their terms are out of the registers while the passes run) */
        if (vB - 1 >= vhor) {
            const float cost_s = unary_cost(P, t.sd, pwih, t.seg_s);
            if (open_s && live && cost_s <= bs) { bs = cost_s; vs = vB; }
        } else {
            const float cost_g = unary_cost(P, t.gd, pwih, t.seg_g);
            if (open_g && live && cost_g <= bg) { bg = cost_g; vg = vB; }
        }
        float lb_o = 0.0f;
        if (prune_on) {
            /* the longest segment of the step: lane 0 (vB = 64 s + 1 <= vT) */
            /* (the long form on purpose: through readfirstlane_f these reads give the kernel other code) */
            const float f_on = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(t.f_on)));
            const float f_oi = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(t.f_oi)));
            const float f_sky = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(t.f_sky)));
            const float f_g = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(t.f_g)));
            /* (wave-uniform, and live across the networks: in an SGPR) */
            lb_o = readfirstlane_f(P.sw * __builtin_fminf(f_on, f_oi - pr.E2) - pr.E1o);
            const float lb_s = P.sw * f_sky - pr.E1s;
            const float lb_g = P.sw * f_g - pr.E1g;
            if (__builtin_amdgcn_ballot_w64(lb_s > bs) != 0ull) open_s = false;
            if (__builtin_amdgcn_ballot_w64(lb_g > bg) != 0ull) open_g = false;
        }
        {
            /* lutT[vB][fni]: one network pass per distinct fn of the live lanes; the first step of the row also
             * leaves lutT[vT + 1][fn] (lane vT - 64 s) in the row cache */
            const int blk = min(2 * s + (lane >> 5), L.nb - 1); /* (clamped: rows >= H only feed dead lanes) */
            const int lT = vT - 64 * s;
            const bool keep_row = s == s_first && lT < 64;
            float ent = 0.0f;
            uint64_t m = __builtin_amdgcn_ballot_w64(live);
            while (m != 0ull) {
                const int fn = __builtin_amdgcn_readlane(t.fni, __builtin_ctzll(m));
                m &= ~__builtin_amdgcn_ballot_w64(t.fni == fn);
                const float out = lut_network(L, disS, fn, blk, lane);
                ent = t.fni == fn ? out : ent;
                if (keep_row) {
                    const float v = readlane_f(out, lT);
                    if (lane == 0) { L.s_tag[fn] = vT + 1; L.s_val[fn] = v; }
                }
            }
            const float od = lut_row_entry(L, disT, vT, t.fni, live, lane) - ent;
            const float cost_o = unary_cost(P, od, pwih, t.seg_o);
            if (live && cost_o <= bo) { bo = cost_o; vo = vB; }
        }
        if (prune_on) {
            /* lb > (the row's best) <=> some lane's best is below lb (a best is never NaN) */
            if (__builtin_amdgcn_ballot_w64(lb_o > bo) != 0ull) open_o = false;
            /* candidates left: vB' <= 64 s; sky ones need vB' - 1 >= vhor */
            const bool sky_left = 64 * s - 1 >= vhor;
            if (!open_o && !open_g && (!open_s || !sky_left)) { ended = true; break; }
        }
    }
    /* The object type is closed for the rest of the row: chunks 0 / 4 / 5 of the vB record instead of the whole of
     * it (chunk 0 only while ground is open), eval_segment's ground and sky terms alone (eval_segment_gs), no table
     * entries; the same bounds for the types still open, the same exit test. */
    for (; s >= 0 && !ended; s--) {
        const int vB = 64 * s + 1 + lane;
        const bool live = vB <= vT;
        const int vBc = live ? vB : vT;
        const int h = vT + 1 - vBc;
        const float pwih = P.pw * rcp[h];
        IS_MY_REC();
        SegTerms t;
        if (open_g) t = eval_segment_gs<IS_WANT_GROUND | IS_WANT_SKY>(my, load_rec_gs<IS_WANT_GROUND | IS_WANT_SKY>(rcol + vBc), P.iw);
        else t = eval_segment_gs<IS_WANT_SKY>(my, load_rec_gs<IS_WANT_SKY>(rcol + vBc), P.iw);
        if (vB - 1 >= vhor) {
            const float cost_s = unary_cost(P, t.sd, pwih, t.seg_s);
            if (open_s && live && cost_s <= bs) { bs = cost_s; vs = vB; }
        } else if (open_g) {
            const float cost_g = unary_cost(P, t.gd, pwih, t.seg_g);
            if (live && cost_g <= bg) { bg = cost_g; vg = vB; }
        }
        /* (prune_on holds: only a bound closes the object type) */
        const float f_sky = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(t.f_sky)));
        const float lb_s = P.sw * f_sky - pr.E1s;
        if (__builtin_amdgcn_ballot_w64(lb_s > bs) != 0ull) open_s = false;
        if (open_g) {
            const float f_g = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(t.f_g)));
            const float lb_g = P.sw * f_g - pr.E1g;
            if (__builtin_amdgcn_ballot_w64(lb_g > bg) != 0ull) open_g = false;
        }
        const bool sky_left = 64 * s - 1 >= vhor;
        if (!open_g && (!open_s || !sky_left)) ended = true;
    }
    /* first segment vB = 0 (:481-594): ground + object, lane 0.  In row 0 it is the only candidate (no step ran: the
     * object type is open, h0 = 1): the same code, once -- a second copy of it costs its spilled SGPRs again. */
    if (!ended) {
        const int h0 = vT + 1;
        const float r0 = rcp[h0];
        const float pwih0 = P.pw * r0;
        IS_MY_REC();
        if (open_o) {
            const RowRec rb0 = rec_of_spread(load_rec_spread(rcol, lane)); /* (the block stays in its VGPRs) */
            const SegTerms t0 = eval_segment<true, HAS_INVALID>(my, rb0, (float)h0, r0, D, P.iw, rcp);
            const float od = lut_row_entry(L, disT, vT, t0.fni, lane == 0, lane) - 0.0f; /* lutT[0] = 0 */
            const float cost_o = unary_cost(P, od, pwih0, t0.seg_o);
            if (lane == 0 && cost_o <= bo) { bo = cost_o; vo = 0; }
            if (open_g) {
                const float cost_g = unary_cost(P, t0.gd, pwih0, t0.seg_g);
                if (lane == 0 && vT <= vhor && cost_g <= bg) { bg = cost_g; vg = 0; }
            }
        } else if (open_g) {
            const SegTerms t0 = eval_segment_gs<IS_WANT_GROUND>(my, load_rec_gs<IS_WANT_GROUND>(rcol), P.iw);
            const float cost_g = unary_cost(P, t0.gd, pwih0, t0.seg_g);
            if (lane == 0 && vT <= vhor && cost_g <= bg) { bg = cost_g; vg = 0; }
        }
    }
    static_assert(IS_GROUND == 0 && IS_OBJECT == 1 && IS_SKY == 2, "the order of unary_merge_lanes' pairs");
    return unary_merge_lanes({bg, bo, bs}, {vg, vo, vs}); /* (wave-uniform) */
#undef IS_MY_REC
}

/* (7 waves per SIMD, 72 VGPRs: what the LDS of 28 waves per CU allows; the held block leaves no slack below it) */
template <bool HAS_INVALID>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(7, 7)))
void k_unary_path(const DevParams P, int ncols, const RowRec* __restrict__ recs, const float* __restrict__ joined,
                  const float* __restrict__ lutC, const float* __restrict__ cost_F, const float* __restrict__ rcp,
                  const int* __restrict__ vhor_arr, const int* __restrict__ col_flags,
                  const PruneRec* __restrict__ prune, float* __restrict__ cost_table,
                  int32_t* __restrict__ index_table, is_section* __restrict__ sections /* or null */,
                  int* __restrict__ bad, int force_bad) {
    const int colg = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (force_bad && colg == 0 && lane == 0) /* (IS_UNARY_PATH=3, tests: distrust every call) */
        __hip_atomic_fetch_or(bad, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (colg >= ncols) return;
    if (__builtin_amdgcn_readfirstlane(col_flags[colg]) != 0) return; /* generic encoding: k_dp_unary */
    const int H = P.H, S = P.S;
    const int vhor = __builtin_amdgcn_readfirstlane(vhor_arr[colg / P.C]);
    const RowRec* rcol = recs + (size_t)colg * (H + 1);
    /* [32]: one record (spread_of_lane), [2][D]: the row cache of lut_row_entry, [S][4]: the chain's hops */
    extern __shared__ __attribute__((aligned(16))) int s_walk[];
    int* s_lut_row = s_walk + 32;
    LutCol L;
    L.H = H; L.D = P.D; L.nb = isk_lut_carry_rows(H);
    L.dcol = joined + (size_t)colg * H;
    L.ccol = lutC + (size_t)colg * L.nb * P.D;
    L.costF = cost_F;
    L.s_tag = s_lut_row;
    L.s_val = (float*)(s_lut_row + P.D);
    for (int i = lane; i < P.D; i += 64) L.s_tag[i] = -1;
    L.s_my = s_walk;
    int* s_cut = s_lut_row + 2 * P.D; /* [S][4]: vT, vB, type, cost bits of every hop (CallPlan::walk_sections) */
    float* ct = cost_table + (size_t)colg * H * 3;
    int32_t* it = index_table + (size_t)colg * H * 3;
    PruneRec pr;
    {
        cprune_t q = (cprune_t)(prune + colg);
        pr.E1o = q->E1o; pr.E1g = q->E1g; pr.E1s = q->E1s; pr.E2 = q->E2;
    }
    /* k_backtrace's walk (is_k_backtrace.hip): the type of the last row, then per Section the arg-min of row
     * vB - 1 with its tie rules; at most S - 1 Sections, and the row vB - 1 of the last one is still read */
    int vT = H - 1, n = 0, type = IS_OBJECT;
    bool last = false;
    int cs = -1; /* the block path_row holds across rows: none yet */
    RowRec cb;
    {
        int* d = (int*)&cb;
#pragma unroll
        for (int i = 0; i < 32; i++) d[i] = 0;
    }
    for (;;) {
        const PathBest b = path_row<HAS_INVALID>(P, rcol, L, rcp, pr, vT, vhor, lane, cs, cb);
        if (lane == 0) {
            ct[vT * 3 + 0] = b.c[0]; ct[vT * 3 + 1] = b.c[1]; ct[vT * 3 + 2] = b.c[2];
            it[vT * 3 + 0] = b.v[0]; it[vT * 3 + 1] = b.v[1]; it[vT * 3 + 2] = b.v[2];
        }
        if (last) break;
        const float cG = b.c[IS_GROUND], cO = b.c[IS_OBJECT], cS = b.c[IS_SKY];
        int t = IS_OBJECT;
        if (cG < cO) t = IS_GROUND;
        if ((n == 0 || type == IS_OBJECT) && cS < __builtin_fminf(cG, cO)) t = IS_SKY;
        type = t;
        const int vB = type == IS_GROUND ? b.v[IS_GROUND] : (type == IS_OBJECT ? b.v[IS_OBJECT] : b.v[IS_SKY]);
        if (vB < 0 || vB > vT) { /* the back-trace would leave the rows this walk can vouch for */
            if (lane == 0) __hip_atomic_fetch_or(bad, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return; /* no Section of this column is written: the ungated k_backtrace of the repair writes them */
        }
        if (sections != nullptr && lane == 0) { /* (n <= S - 2) */
            const float c = type == IS_GROUND ? cG : (type == IS_OBJECT ? cO : cS);
            s_cut[4 * n + 0] = vT; s_cut[4 * n + 1] = vB; s_cut[4 * n + 2] = type; s_cut[4 * n + 3] = __float_as_int(c);
        }
        n++;
        if (vB == 0) break;
        vT = vB - 1;
        last = n >= S - 1;
    }
    if (sections == nullptr) return;
    /* the chain succeeded: the lanes build its n Sections and the terminator, as k_backtrace's second loop does */
    __syncthreads(); /* (one wave) lane 0's hops before the lanes read them */
    is_section* out = sections + (size_t)colg * S;
    for (int i0 = 0; i0 <= n; i0 += 64) {
        const int i = i0 + lane;
        is_section sec;
        sec.type = -1; sec.vB = 0; sec.vT = 0; sec.disparity = 0.0f; /* terminator, :952-954 */
        sec.semantic_class = 0; sec.cost = 0.0f; sec.instance_meanx = 0.0f; sec.instance_meany = 0.0f;
        if (i < n)
            sec = make_section(P, rcol, false, s_cut[4 * i + 0], s_cut[4 * i + 1], s_cut[4 * i + 2],
                               __int_as_float(s_cut[4 * i + 3]));
        if (i <= n) out[i] = sec;
    }
}

/* The instantiation for (invalid-disparity value or none) */
static decltype(&k_unary_path<false>) unary_path_kernel(bool invalid) {
    return invalid ? k_unary_path<true> : k_unary_path<false>;
}

extern "C" {

/* one record, the row cache [2][D] and the hops [S][4] */
size_t isk_unary_path_lds_bytes(const DevParams* P) {
    return sizeof(int) * (2 * (size_t)P->D + 4 * (size_t)P->S + 32);
}

hipError_t isk_set_lds_unary_path(const DevParams* P) {
    return hipFuncSetAttribute((const void*)unary_path_kernel(P->invalid >= 0), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)isk_unary_path_lds_bytes(P));
}

hipError_t isk_launch_unary_path(const DevParams* P, const CallPlan* plan, const CallBuffers* b, hipStream_t stream) {
    hipLaunchKernelGGL(unary_path_kernel(P->invalid >= 0), dim3(plan->ncols), dim3(64), isk_unary_path_lds_bytes(P), stream,
                       *P, plan->ncols, b->recs, b->joined, b->lutC, b->cost_F, b->rcp, b->vhor, b->col_flags, b->prune,
                       b->cost_table, b->index_table, plan->walk_sections ? b->sections : nullptr, b->path_bad,
                       plan->unary_force_bad);
    return hipGetLastError();
}

} /* extern "C" */
