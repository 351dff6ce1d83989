/* is_k_prepare.hip -- per-column boundary records, object data-cost prefix table, pairwise
 * prior tables.  See is_kernels.h. */
#include "is_kernels.h"

/* ====================================================================================== */
/* A4-A6  per-column preparation                                                           */
/* ====================================================================================== */
#define PREP_THREADS 256
#define PREP_MAXR 9 /* rows per thread whose fp32 prefixes are held in registers: H + 1 <= 9 * 256 */

/* LDS stride of a segmentation channel: H/8 + 1 prefix entries, rounded up to 16 bytes */
__host__ __device__ static constexpr int prep_seg_stride(int H) { return (((H >> 3) + 1) + 3) & ~3; }
/* leaves of the fp32 scan trees: H when H is a power of two (then P2 = 2H), else P2 */
__host__ __device__ static constexpr int prep_scan_leaves(int H, int P2) {
    return ((H & (H - 1)) == 0 && P2 == 2 * H && H >= 16) ? H : P2;
}
/* DevParams::P2 of a context of H rows: the smallest power of two >= H + 1 (is_ctx_create), and the log2 of one */
__host__ __device__ static constexpr int prep_rows_pow2(int H) {
    int p = 1;
    while (p < H + 1) p <<= 1;
    return p;
}
__host__ __device__ static constexpr int prep_log2(int pow2) {
    int l = 0;
    while ((1 << l) < pow2) l++;
    return l;
}

/* Exclusive prefix of index i (0 <= i < n) with the association of the reference's
 * work-efficient block scan ComputePrefixSum (StixelsKernels.h:73-103): the up-sweep builds a
 * pairwise tree, the down-sweep gives a right child `parent + left subtree sum`, i.e. the
 * left-sibling sums on the root-to-leaf path are added top-down starting from 0.
 * pyr holds the tree: level b (n>>b nodes) at offset 2n - (2n>>b). */
__device__ __forceinline__ float blelloch_prefix(const float* pyr, int n, int log2n, int i) {
    float acc = 0.0f;
    for (int b = log2n - 1; b >= 0; b--) {
        const int node = i >> b;
        if (node & 1) acc = acc + pyr[(2 * n - ((2 * n) >> b)) + node - 1];
    }
    return acc;
}

__device__ __forceinline__ void blelloch_build(float* pyr, int n, int log2n) {
    for (int b = 1; b <= log2n; b++) {
        const float* lo = pyr + (2 * n - ((2 * n) >> (b - 1)));
        float* hi = pyr + (2 * n - ((2 * n) >> b));
        for (int j = threadIdx.x; j < (n >> b); j += PREP_THREADS) hi[j] = lo[2 * j + 1] + lo[2 * j];
        __syncthreads();
    }
}

/* Exact exclusive block scan of one int64 per thread (any association is exact). */
__device__ __forceinline__ int64_t block_excl_scan_i64(int64_t v, int64_t* s_wave /*[4]*/) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t inc = v;
#pragma unroll
    for (int j = 1; j < 64; j <<= 1) {
        const int64_t n = __shfl_up(inc, j, 64);
        if (lane >= j) inc += n;
    }
    __syncthreads(); /* s_wave may still be read by the previous call */
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int64_t base = 0;
    for (int w = 0; w < wave; w++) base += s_wave[w];
    return base + inc - v;
}

/* Block totals of N 64-bit values per thread, through s_abs (N <= 4 words that alias s_wave).  Three barriers: the
 * zeroes, the sums, and the last one frees the words for their next user. */
template <int N>
__device__ __forceinline__ void block_sum_u64(unsigned long long (&v)[N], unsigned long long* s_abs) {
    if (threadIdx.x < N) s_abs[threadIdx.x] = 0ull;
    __syncthreads();
#pragma unroll
    for (int n = 0; n < N; n++) atomicAdd(&s_abs[n], v[n]);
    __syncthreads();
#pragma unroll
    for (int n = 0; n < N; n++) v[n] = s_abs[n];
    __syncthreads();
}

/* (sum, min) over the block; s_red holds 8 floats.  Only used for slack bounds (PruneRec), which
 * carry their own safety factor, so the summation order does not matter. */
__device__ __forceinline__ float2 block_sum_min(float s, float m, float* s_red) {
#pragma unroll
    for (int j = 32; j >= 1; j >>= 1) {
        s += __shfl_xor(s, j, 64);
        m = __builtin_fminf(m, __shfl_xor(m, j, 64));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) { s_red[wave] = s; s_red[4 + wave] = m; }
    __syncthreads();
    float2 r;
    r.x = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
    r.y = __builtin_fminf(__builtin_fminf(s_red[4], s_red[5]), __builtin_fminf(s_red[6], s_red[7]));
    return r;
}

__device__ __forceinline__ float data_cost_sky(float d, const DevParams& P) {
    /* GetDataCostSky, StixelsKernels.cu:201-215 */
    float data_cost = P.pnex_sky_log;
    if (d != P.invalid) {
        const float pgaussian = P.norm_sky + d * d * P.inv_sigma2_sky;
        const float p_data = __builtin_fminf(P.puniform_sky, pgaussian);
        data_cost = p_data + P.nopnex_sky_log;
    }
    return data_cost;
}
__device__ __forceinline__ float data_cost_ground(float fn, float d, float norm_g, float inv_s2_g,
                                                  const DevParams& P) {
    /* GetDataCostGround, StixelsKernels.cu:217-234 */
    float data_cost = P.pnex_gnd_log;
    if (d != P.invalid) {
        const float model_diff = (d - fn);
        const float pgaussian = norm_g + model_diff * model_diff * inv_s2_g;
        const float p_data = __builtin_fminf(P.puniform, pgaussian);
        data_cost = p_data + P.nopnex_gnd_log;
    }
    return data_cost;
}

/* The LDS of a column's workgroup.  Reuse, in the order of prepare_columns_body: `seg` holds the raw channels, then
 * the offset channels squared in place, then every channel's exclusive prefix in place; `wave` serves block_sum_u64
 * (as s_abs) and block_excl_scan_i64 in turn; `pyr` is refilled for each of the four fp32 planes. */
struct PrepLds {
    float* d;      /* [NP]     disparity column, zero beyond H                        */
    float* pyr;    /* [2 * NP] scan tree                                              */
    int32_t* seg;  /* [CH][SS] segmentation channels at 1/8 resolution                */
    int64_t* wave; /* [4]      wave totals of the int64 scans / s_abs of the block sums */
    float* red;    /* [8]      block_sum_min                                          */
    float* tot;    /* [2]      tot[0] = sum mx^2 + my^2 of the column                 */
};
#define PREP_LDS_TAIL 192 /* wave + red + tot: 72 bytes, with room to the next 64 */
__device__ __forceinline__ PrepLds prep_lds(char* smem, int NP, int CH, int SS) {
    float* d = (float*)smem;
    int32_t* seg = (int32_t*)(d + 3 * NP);
    int64_t* wave = (int64_t*)(seg + CH * SS);
    return {d, d + NP, seg, wave, (float*)(wave + 4), (float*)(wave + 4) + 8};
}
/* bytes of that carve-up */
__host__ __device__ static constexpr size_t prep_lds_carve_bytes(int NP, int CH, int SS) {
    return sizeof(float) * (size_t)NP * 3 + sizeof(int32_t) * (size_t)CH * SS + PREP_LDS_TAIL;
}
extern "C" size_t isk_prepare_lds_bytes(const DevParams* P) {
    return prep_lds_carve_bytes(prep_scan_leaves(P->H, P->P2), P->CH, prep_seg_stride(P->H));
}

/* What the stages of one column share: its shape, which column it is, who owns which rows, where its data lie.
 * PrepCol<HC>, HC > 0: a kernel compiled for HC rows -- everything that follows from the row count alone is a constant
 * of the type (the same names, so the stages read c.H, c.NP, .. either way); PrepCol<0>: the rows at run time. */
struct PrepColWhere {
    int K, CH;
    int colg, img, col, tid;
    int r_lo;            /* instance sums: thread t owns rows [t * R, t * R + R) */
    const int32_t* scol; /* [CH][P2S]  its segmentation channels */
    RowRec* rcol;        /* [H + 1]    its records               */
};
template <int HC>
struct PrepCol : PrepColWhere {
    static constexpr int H = HC, SS = prep_seg_stride(HC);
    static constexpr int P2 = prep_rows_pow2(HC), NP = prep_scan_leaves(HC, P2), LNP = prep_log2(NP);
    static constexpr int R = (HC + PREP_THREADS - 1) / PREP_THREADS;
    static constexpr bool regs = (HC + 1) <= PREP_MAXR * PREP_THREADS;
    /* live slots of PrepPlanes and blocks of the epilogue: rows 0 .. H */
    static constexpr int slots = regs ? (HC + 1 + PREP_THREADS - 1) / PREP_THREADS : 0;
};
template <>
struct PrepCol<0> : PrepColWhere {
    int H;
    /* LDS stride of a segmentation channel: only its first H/8 + 1 entries matter (an exclusive prefix at index <= H/8
     * never sees the zero padding up to P2S), and 21 channels of P2S = 256 entries were 21.5 of the kernel's 46 KB of
     * LDS: with 132 the CU holds four workgroups, not three */
    int SS;
    /* The scans run over P2 >= H + 1 zero-padded elements (StixelsKernels.h:73-103).  When H is a power of two (P2 =
     * 2H) everything a prefix at index <= H needs lies in the LEFT half of that tree: indices < H walk the same nodes
     * as in a tree over H leaves, and index H is the left child of the root = the root of the H-leaf tree.  The tree is
     * then built over NP = H leaves: identical sums, half the LDS (12 instead of 24 KB at H = 1024). */
    int NP, LNP;
    int R; /* rows per thread of the instance sums (r_lo) */
    /* fp32 prefixes: thread t owns rows t + k * PREP_THREADS.  regs: it keeps them in registers (PrepPlanes) and the
     * records get {G, K, S, V} as ONE 16-byte store per row at the end, block by block (prep_store_records); else each
     * prefix goes to its record field at once */
    bool regs;
    static constexpr int slots = PREP_MAXR; /* each guarded by the row count */
};
/* the shapes a kernel is compiled for: the benchmarked row counts (the headline shape, ref_shape_784x1792) */
static_assert(PrepCol<1024>::NP == 1024 && PrepCol<1024>::LNP == 10 && PrepCol<1024>::slots == 5, "1024 rows");
static_assert(PrepCol<784>::NP == 1024 && PrepCol<784>::LNP == 10 && PrepCol<784>::slots == 4, "784 rows");
template <int HC>
__device__ __forceinline__ PrepCol<HC> prep_col(const DevParams& P, int colg, const int32_t* seg, RowRec* recs) {
    PrepCol<HC> c;
    if constexpr (HC == 0) {
        c.H = P.H;
        c.SS = prep_seg_stride(c.H);
        c.NP = prep_scan_leaves(c.H, P.P2);
        c.LNP = (c.NP == P.P2) ? P.log2P2 : P.log2P2 - 1;
        c.R = (c.H + PREP_THREADS - 1) / PREP_THREADS;
        c.regs = (c.H + 1) <= PREP_MAXR * PREP_THREADS;
    }
    c.K = P.K, c.CH = P.CH;
    c.colg = colg, c.img = colg / P.C, c.col = colg % P.C, c.tid = threadIdx.x;
    c.r_lo = c.tid * c.R;
    c.scol = seg + (size_t)colg * c.CH * P.P2S;
    c.rcol = recs + (size_t)colg * (c.H + 1);
    return c;
}

/* ---- the column inputs into LDS with 16-byte loads (H is a multiple of 8; the segmentation column is
 * 16-byte aligned when P2S is a multiple of 4) */
template <int HC>
__device__ __forceinline__ void prep_stage_column(const DevParams& P, const PrepLds& L, const PrepCol<HC>& c,
                                                  const float* __restrict__ joined) {
    const int H = c.H, SS = c.SS, CH = c.CH, P2S = P.P2S, tid = c.tid;
    const float4* d4 = reinterpret_cast<const float4*>(joined + (size_t)c.colg * H);
    float4* sd4 = reinterpret_cast<float4*>(L.d);
    for (int i = tid; i < (H >> 2); i += PREP_THREADS) sd4[i] = d4[i];
    for (int i = H + tid; i < c.NP; i += PREP_THREADS) L.d[i] = 0.0f;
    if ((P2S & 3) == 0 && SS <= P2S) {
        const int4* g4 = reinterpret_cast<const int4*>(c.scol);
        int4* s4 = reinterpret_cast<int4*>(L.seg);
        const int sq = SS >> 2, gq = P2S >> 2;
#pragma unroll 4
        for (int i = tid; i < CH * sq; i += PREP_THREADS) {
            const int ch = i / sq, q = i - ch * sq;
            s4[i] = g4[ch * gq + q];
        }
    } else {
        for (int i = tid; i < CH * SS; i += PREP_THREADS) {
            const int ch = i / SS, k = i - ch * SS;
            L.seg[i] = k < P2S ? c.scol[ch * P2S + k] : 0;
        }
    }
}

/* ---- fn windows of the pairwise phase 1 (is_device.h, IS_P1_WIN): per 64-row tile the smallest valid
 * disparity, rounded down to a multiple of 4 columns (16-byte loads), one below for the rounding of
 * the prefix sums a mean is computed from.  Reads L.d. */
template <int HC>
__device__ __forceinline__ void prep_fn_windows(const DevParams& P, const PrepLds& L, const PrepCol<HC>& c) {
    if (!(IS_P1_WINDOWED(P.D) && P.win_lo != nullptr)) return;
    const int lane = c.tid & 63, wv = c.tid >> 6;
    for (int t = wv; t < P.ntiles; t += PREP_THREADS / 64) {
        const int r = t * 64 + lane;
        float d = IS_INF, dx = -IS_INF;
        bool ok = false;
        if (r < c.H) {
            const float x = L.d[r];
            if (!(P.invalid >= 0 && x == P.invalid) && x == x) { d = dx = x; ok = true; }
        }
        const float mine = d;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            d = __builtin_fminf(d, __shfl_xor(d, m, 64));
            dx = __builtin_fmaxf(dx, __shfl_xor(dx, m, 64));
        }
        /* three candidates: the contiguous window that starts at the tile's smallest disparity (the segments of
         * a lane start below its row -- nearer, larger disparities), the contiguous one that ends at its largest,
         * and the SPLIT one: half A from the smallest disparity on, half B up to the largest -- a tile above the
         * horizon can hold sky (d ~ 0) AND an object.  Whichever holds most of the tile's rows (ties: contiguous). */
        constexpr int HW = IS_WIN_HALF;
        int lo_a = 0, lo_b = 0, hi_b = 0;
        if (d < IS_INF) {
            lo_a = (int)__builtin_fminf(__builtin_fmaxf(d, 1.0f), (float)P.D) - 1;
            lo_b = (int)__builtin_fminf(__builtin_fmaxf(dx, 0.0f), (float)(P.D - 1)) + 2 - IS_P1_WIN;
            hi_b = (int)__builtin_fminf(__builtin_fmaxf(dx, 0.0f), (float)(P.D - 1)) + 2 - HW;
        }
        lo_a = min(max(lo_a, 0) & ~3, P.D - IS_P1_WIN);
        lo_b = min(max(lo_b, 0) & ~3, P.D - IS_P1_WIN);
        hi_b = min(max(hi_b, 0) & ~3, P.D - HW);
        const int w_a = IS_WIN_PACK(lo_a, lo_a + HW), w_b = IS_WIN_PACK(lo_b, lo_b + HW);
        const int w_s = IS_WIN_PACK(lo_a, max(hi_b, lo_a + HW)); /* (never overlapping halves) */
        const int fl = (int)__builtin_fminf(__builtin_fmaxf(mine, 0.0f), (float)(P.D - 1));
        const int n_a = __builtin_popcountll(__builtin_amdgcn_ballot_w64(ok && IS_WIN_FIND(w_a, fl) >= 0));
        const int n_b = __builtin_popcountll(__builtin_amdgcn_ballot_w64(ok && IS_WIN_FIND(w_b, fl) >= 0));
        const int n_s = __builtin_popcountll(__builtin_amdgcn_ballot_w64(ok && IS_WIN_FIND(w_s, fl) >= 0));
        int w_best = n_b > n_a ? w_b : w_a;
        if (n_s > max(n_a, n_b)) w_best = w_s;
        if (lane == 0) P.win_lo[(size_t)c.colg * P.ntiles + t] = w_best;
    }
}

/* Running sums of the instance-centre values of a column's rows (StixelsKernels.cu:401-409): the squares in wrapping
 * 64-bit arithmetic. */
struct InstSums { int64_t mx, my, mx2, my2; };
/* The instance centre (mx, my) of row r from the RAW offset values of its 1/8-resolution block, added to s.
 * mx = 8*col + 3.5 + offx + 0.5 is an exact integer; my = trunc(row - offy + 0.5): n for n >= 0, n + 1 for n < 0
 * (truncation toward zero). */
__device__ __forceinline__ void instance_centre_add(const DevParams& P, int col, int r, int32_t offx, int32_t offy,
                                                    InstSums& s, int64_t& mx, int64_t& my) {
    const double fx = ((double)(P.column_step * col) + 0.5 * ((double)P.column_step - 1.0)) + (double)offx + 0.5;
    mx = (int64_t)fx;
    const int32_t n32 = (int32_t)((uint32_t)r - (uint32_t)offy);
    my = (int64_t)((double)n32 + 0.5);
    s.mx += mx;
    s.my += my;
    s.mx2 = (int64_t)((uint64_t)s.mx2 + (uint64_t)mx * (uint64_t)mx);
    s.my2 = (int64_t)((uint64_t)s.my2 + (uint64_t)my * (uint64_t)my);
}

/* ---- instance sums of this thread's rows and the three checks of the FAST encodings (RowRec).  Returns `slow`, the
 * same in every thread: the column needs the generic (int64 / IEEE-division) DP path; `base`: the exclusive prefixes of
 * the four sums at row r_lo; L.tot[0]: the column totals of the squares.  L.wave: block_sum_u64, then the four scans. */
template <int HC>
__device__ __forceinline__ int prep_instance_sums(const DevParams& P, const PrepLds& L, const PrepCol<HC>& c,
                                                  int* __restrict__ col_flags, int* __restrict__ n_generic,
                                                  InstSums& base) {
    const int H = c.H, K = c.K, SS = c.SS, tid = c.tid;
    const int32_t* offy = L.seg + K * SS;
    const int32_t* offx = L.seg + (K + 1) * SS;
    InstSums sum = {0, 0, 0, 0};
    unsigned long long abs_m[2] = {0ull, 0ull};
    int slow = 0;
    for (int r = c.r_lo; r < c.r_lo + c.R && r < H; r++) {
        int64_t mx, my;
        instance_centre_add(P, c.col, r, offx[r >> 3], offy[r >> 3], sum, mx, my);
        abs_m[0] += (uint64_t)(mx < 0 ? -mx : mx);
        abs_m[1] += (uint64_t)(my < 0 ? -my : my);
        const float ad = __builtin_fabsf(L.d[r]);
        slow |= !((ad == 0.0f) || (ad >= IS_FAST_DISP_MIN && ad <= IS_FAST_DISP_MAX));
    }
    /* instance centres of a FAST column: sum|mx|, sum|my| < 2^23 */
    block_sum_u64(abs_m, (unsigned long long*)L.wave);
    slow |= (abs_m[0] >= (unsigned long long)IS_FAST_INSTANCE_LIMIT) |
            (abs_m[1] >= (unsigned long long)IS_FAST_INSTANCE_LIMIT);
    { /* class channels of a FAST column: values >= 0, full-resolution total < 2^24.  One wave per channel (round
       * robin), a lane sums every 64th entry, the wave adds the lane sums (the nineteen channels used to be walked by
       * nineteen lanes of wave 0: 132 serial iterations with an integer modulo each, a tenth of the workgroup's life) */
        const int lane = tid & 63, wv = tid >> 6;
        for (int ch = wv; ch < K; ch += PREP_THREADS / 64) {
            const int32_t* p = L.seg + ch * SS;
            uint64_t total = 0;
            int negative = 0;
            for (int k = lane; k < SS; k += 64) {
                const int32_t x = p[k];
                negative |= (x < 0);
                total += (uint64_t)(uint32_t)x;
            }
#pragma unroll
            for (int j = 32; j >= 1; j >>= 1) {
                total += (uint64_t)__shfl_xor((unsigned long long)total, j, 64);
                negative |= __shfl_xor(negative, j, 64);
            }
            slow |= negative | (total * IS_DOWNSAMPLE_FACTOR >= (uint64_t)IS_FAST_CLASS_LIMIT);
        }
    }
    slow = __syncthreads_or(slow);
    if (tid == 0) {
        col_flags[c.colg] = slow;
        if (slow) atomicAdd(n_generic, 1); /* (zeroed by the caller before the launch) */
    }
    base.mx = block_excl_scan_i64(sum.mx, L.wave);
    base.my = block_excl_scan_i64(sum.my, L.wave);
    base.mx2 = block_excl_scan_i64(sum.mx2, L.wave);
    base.my2 = block_excl_scan_i64(sum.my2, L.wave);
    /* the column totals (PruneRec.E2): the owner of row H - 1 has them, its exclusive prefix + its own rows -- the
     * integers prep_store_instance_rows will end with */
    if (c.r_lo <= H - 1 && H - 1 < c.r_lo + c.R)
        L.tot[0] = (float)((double)(int64_t)((uint64_t)base.mx2 + (uint64_t)sum.mx2) +
                           (double)(int64_t)((uint64_t)base.my2 + (uint64_t)sum.my2));
    return slow;
}

/* ---- square the offset channels of L.seg in place (StixelsKernels.cu:411-416).  Returns nic_bad, the same in every
 * thread: the branch-and-bound precondition fails.  The non-instance offset term is >= 0 and monotone when no
 * squared entry is negative as int32 (the reference squares in wrapping int32) and the full-resolution total stays
 * below 2^31.  L.wave: block_sum_u64. */
template <int HC>
__device__ __forceinline__ int prep_square_offsets(const PrepLds& L, const PrepCol<HC>& c) {
    int32_t* off = L.seg + c.K * c.SS; /* offy, then offx */
    for (int i = c.tid; i < 2 * c.SS; i += PREP_THREADS) {
        const uint32_t x = (uint32_t)off[i];
        off[i] = (int32_t)(x * x);
    }
    __syncthreads();
    int nic_bad = 0;
    unsigned long long sq_sum[1] = {0ull};
    for (int i = c.tid; i < 2 * c.SS; i += PREP_THREADS) {
        const int32_t v = off[i];
        nic_bad |= v < 0;
        sq_sum[0] += (unsigned long long)(uint32_t)v;
    }
    block_sum_u64(sq_sum, (unsigned long long*)L.wave);
    nic_bad |= (sq_sum[0] * IS_DOWNSAMPLE_FACTOR) >= (1ull << 31);
    return __syncthreads_or(nic_bad);
}

/* ---- every channel of L.seg becomes its exclusive prefix at 1/8 resolution, in place (:462-469); integer, so any
 * order is exact.  One wave per channel (round robin): lane l owns `per` consecutive entries of the SS */
template <int HC>
__device__ __forceinline__ void prep_class_prefixes(const PrepLds& L, const PrepCol<HC>& c) {
    const int SS = c.SS, lane = c.tid & 63, wv = c.tid >> 6, per = (SS + 63) >> 6;
    for (int chn = wv; chn < c.CH; chn += PREP_THREADS / 64) {
        int32_t* ch = L.seg + chn * SS;
        uint32_t local = 0;
        for (int k = 0; k < per; k++) {
            const int idx = lane * per + k;
            if (idx < SS) local += (uint32_t)ch[idx];
        }
        uint32_t inc = local; /* inclusive wave scan of the lane totals */
#pragma unroll
        for (int j = 1; j < 64; j <<= 1) {
            const uint32_t n = (uint32_t)__shfl_up((int)inc, j, 64);
            if (lane >= j) inc += n;
        }
        uint32_t run = inc - local;
        for (int k = 0; k < per; k++) {
            const int idx = lane * per + k;
            if (idx < SS) {
                const uint32_t x = (uint32_t)ch[idx];
                ch[idx] = (int32_t)run;
                run += x;
            }
        }
    }
}

/* ---- fp32 prefixes with the reference's block-scan association (:452-461): the four planes of a column.  A call
 * site fills L.pyr with the plane's NP values; prep_scan_plane syncs, builds the tree and delivers the prefixes of this
 * thread's rows v = tid + k * PREP_THREADS <= H: into p[k] (c.regs), else into the record field `field`; and into
 * copy[v] where a compact copy is wanted (the S / V copies of the pairwise phase 2).  The caller puts a barrier in
 * front of the next fill. */
struct PrepPlanes { float G[PREP_MAXR], K[PREP_MAXR], S[PREP_MAXR], V[PREP_MAXR]; }; /* this thread's prefixes */
template <int HC>
__device__ __forceinline__ void prep_scan_plane(const PrepLds& L, const PrepCol<HC>& c, float (&p)[PREP_MAXR],
                                                float RowRec::*field, float* __restrict__ copy) {
    const int NP = c.NP, LNP = c.LNP, H = c.H;
    __syncthreads();
    blelloch_build(L.pyr, NP, LNP);
    auto prefix_at = [&](int v) -> float { /* exclusive prefix at v <= H */
        return (v == NP) ? L.pyr[2 * NP - 2] : blelloch_prefix(L.pyr, NP, LNP, v);
    };
    if (c.regs) {
#pragma unroll
        for (int k = 0; k < c.slots; k++) {
            const int v = c.tid + k * PREP_THREADS;
            if (v <= H) { p[k] = prefix_at(v); if (copy) copy[v] = p[k]; }
        }
    } else {
        for (int v = c.tid; v <= H; v += PREP_THREADS) {
            const float x = prefix_at(v);
            c.rcol[v].*field = x;
            if (copy) copy[v] = x;
        }
    }
}

/* S: disparity (valid-masked when invalid >= 0, :382-389) */
template <int HC>
__device__ __forceinline__ void prep_fill_S(const DevParams& P, const PrepLds& L, const PrepCol<HC>& c) {
    for (int i = c.tid; i < c.NP; i += PREP_THREADS) {
        float x = 0.0f;
        if (i < c.H) {
            const float d = L.d[i];
            if (P.invalid >= 0) {
                const int va = d != P.invalid;
                x = ((float)va) * d;
            } else {
                x = d;
            }
        }
        L.pyr[i] = x;
    }
}
/* V: valid count (only with an invalid-disparity value) */
template <int HC>
__device__ __forceinline__ void prep_fill_V(const DevParams& P, const PrepLds& L, const PrepCol<HC>& c) {
    for (int i = c.tid; i < c.NP; i += PREP_THREADS) L.pyr[i] = (i < c.H) ? (float)(L.d[i] != P.invalid) : 0.0f;
}
/* G: ground data cost, +inf at / above the horizon (:435-446).  Returns (sum |x|, min x) over the finite rows: the
 * slack of the ground data term */
template <int HC>
__device__ __forceinline__ float2 prep_fill_G(const DevParams& P, const PrepLds& L, const PrepCol<HC>& c,
                                              const float* __restrict__ ground /*[img][3][H]*/, int vhor) {
    const float* gfun = ground + (size_t)c.img * 3 * c.H;
    const float* gnorm = gfun + c.H;
    const float* gis2 = gnorm + c.H;
    float g_abs = 0.0f, g_min = 0.0f;
    for (int i = c.tid; i < c.NP; i += PREP_THREADS) {
        float x = 0.0f;
        if (i < c.H) {
            x = (i >= vhor) ? IS_INF : data_cost_ground(gfun[i], L.d[i], gnorm[i], gis2[i], P);
            if (i < vhor) { g_abs += __builtin_fabsf(x); g_min = __builtin_fminf(g_min, x); }
        }
        L.pyr[i] = x;
    }
    return block_sum_min(g_abs, g_min, L.red);
}
/* K: sky data cost, 0 below the horizon (:424-433).  Returns (sum |x|, min x) */
template <int HC>
__device__ __forceinline__ float2 prep_fill_K(const DevParams& P, const PrepLds& L, const PrepCol<HC>& c, int vhor) {
    float k_abs = 0.0f, k_min = 0.0f;
    for (int i = c.tid; i < c.NP; i += PREP_THREADS) {
        float x = 0.0f;
        if (i < c.H) x = (i < vhor) ? 0.0f : data_cost_sky(L.d[i], P);
        k_abs += __builtin_fabsf(x);
        k_min = __builtin_fminf(k_min, x);
        L.pyr[i] = x;
    }
    return block_sum_min(k_abs, k_min, L.red);
}

/* ---- PruneRec of the column (thread 0): see is_device.h.  A prefix difference P[a] - P[b] of per-row values x >= -nu
 * with sum|x| = T is >= -(nu * H + gamma2 * T); NaN anywhere makes the slack NaN, and a NaN slack makes every bound
 * NaN, which never passes the `>` test: no pruning.  Reads L.tot[0]. */
template <int HC>
__device__ __forceinline__ void prep_prune_rec(const DevParams& P, const PrepLds& L, const PrepCol<HC>& c, float2 g_red,
                                               float2 k_red, int slow, int nic_bad, PruneRec* __restrict__ prune) {
    if (c.tid != 0) return;
    const float safe = 1.0f + 0x1p-10f;
    const float hf = (float)c.H;
    const float sig_g = ((0.0f - g_red.y) * hf + P.gamma2 * g_red.x) * safe;
    const float sig_k = ((0.0f - k_red.y) * hf + P.gamma2 * k_red.x) * safe;
    PruneRec pr;
    pr.E1o = P.dw * P.sigma_od;
    pr.E1g = P.dw * sig_g;
    pr.E1s = P.dw * sig_k;
    pr.E2 = P.iw * (0x1p-21f * safe) * L.tot[0]; /* 8 * 2^-24 * (sum mx^2 + sum my^2) */
    /* 0 * inf above would be NaN = off as well; make the "off" states explicit */
    if (slow || nic_bad || !(P.sigma_od < IS_INF) || !(pr.E1g < IS_INF) || !(pr.E1s < IS_INF) ||
        !(pr.E2 < IS_INF))
        pr.E1o = pr.E1g = pr.E1s = IS_INF; /* every type: the bounds are tested one by one */
    pr.pad[0] = pr.pad[1] = pr.pad[2] = pr.pad[3] = 0.0f;
    prune[c.colg] = pr;
}

/* ---- the pieces of a 128-byte record, each a 16-byte store: dwords 0..19 the class chunks, 20..23 {G, K, S, V},
 * 24..31 the instance prefixes */
__device__ __forceinline__ void store_gksv(RowRec* o, float g, float k, float s, float v) {
    reinterpret_cast<int4*>(o)[5] = make_int4(__float_as_int(g), __float_as_int(k), __float_as_int(s), __float_as_int(v));
}
__device__ __forceinline__ void store_instance_prefix(RowRec* o, int slow, const InstSums& s) {
    int4 a, b;
    if (slow) { /* RowRecWide: four int64 */
        a = make_int4((int)(uint32_t)s.mx, (int)(uint32_t)((uint64_t)s.mx >> 32), (int)(uint32_t)s.my,
                      (int)(uint32_t)((uint64_t)s.my >> 32));
        b = make_int4((int)(uint32_t)s.mx2, (int)(uint32_t)((uint64_t)s.mx2 >> 32), (int)(uint32_t)s.my2,
                      (int)(uint32_t)((uint64_t)s.my2 >> 32));
    } else { /* exact fp32 encodings, see RowRec */
        const int64_t lo_mask = ((int64_t)1 << IS_FAST_SPLIT_BITS) - 1;
        a = make_int4(__float_as_int((float)s.mx), __float_as_int((float)s.my),
                      __float_as_int((float)(s.mx2 - (s.mx2 & lo_mask))), __float_as_int((float)(s.mx2 & lo_mask)));
        b = make_int4(__float_as_int((float)(s.my2 - (s.my2 & lo_mask))), __float_as_int((float)(s.my2 & lo_mask)),
                      0, 0);
    }
    int4* d = reinterpret_cast<int4*>(o);
    d[6] = a;
    d[7] = b;
}
/* The instance prefixes of this thread's rows [r_lo, r_lo + R): the exclusive prefix at those indices; the owner of
 * row H - 1 also writes index H (the total).  (The raw offsets from the input tensor: the LDS copies have been squared
 * in place.) */
template <int HC>
__device__ __forceinline__ void prep_store_instance_rows(const DevParams& P, const PrepCol<HC>& c, int slow,
                                                         const InstSums& base) {
    const int H = c.H;
    const int32_t* offy = c.scol + c.K * P.P2S;
    const int32_t* offx = c.scol + (c.K + 1) * P.P2S;
    InstSums b = base;
    for (int r = c.r_lo; r < c.r_lo + c.R && r < H; r++) {
        store_instance_prefix(c.rcol + r, slow, b);
        int64_t mx, my;
        instance_centre_add(P, c.col, r, offx[r >> 3], offy[r >> 3], b, mx, my);
    }
    if (c.r_lo <= H - 1 && H - 1 < c.r_lo + c.R) store_instance_prefix(c.rcol + H, slow, b);
}
/* Chunk q (0..4) of dwords 0..19 (class prefixes + squared-offset prefix) of the EIGHT rows of the 1/8-resolution
 * block kb: the full-resolution prefix at row 8 kb + m is ps[kb] * 8 + (ps[kb + 1] - ps[kb]) * m in wrapping uint32
 * arithmetic, so the two table entries are read once per block and the rows follow by repeated addition -- an eighth of
 * the LDS reads and a fifth of the instructions of one (row, chunk) item per thread. */
template <int HC>
__device__ __forceinline__ void prep_store_class_item(const PrepLds& L, const PrepCol<HC>& c, int slow, int kb, int q) {
    const int SS = c.SS, K = c.K;
    const int kn = min(kb + 1, SS - 1); /* (the last block has one row: its increment is never used) */
    uint32_t cur[4], dif[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int dw = q * 4 + j; /* dword of RowRec: Fg0 Fg1 Fon[8] Foi[8] Fsky Fnic */
        if (dw == 19) {
            const int32_t* px = L.seg + (K + 1) * SS;
            const int32_t* py = L.seg + K * SS;
            const uint32_t ax = (uint32_t)px[kb], ay = (uint32_t)py[kb];
            cur[j] = ax * 8u + ay * 8u;
            dif[j] = ((uint32_t)px[kn] - ax) + ((uint32_t)py[kn] - ay);
        } else {
            const int chn = dw < 10 ? dw : (dw < 18 ? dw + 1 : 10);
            const int32_t* ps = L.seg + chn * SS;
            const uint32_t a = (uint32_t)ps[kb];
            cur[j] = a * 8u;
            dif[j] = (uint32_t)ps[kn] - a;
        }
    }
    const bool is_count = (q == 4); /* dword 19 (Fnic) stays an integer in both encodings */
#pragma unroll
    for (int m = 0; m < 8; m++) {
        const int v = kb * 8 + m;
        if (v <= c.H) {
            int32_t x[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int32_t f = (int32_t)cur[j];
                x[j] = (slow || (is_count && j == 3)) ? f : __float_as_int((float)f);
                cur[j] += dif[j];
            }
            reinterpret_cast<int4*>(c.rcol + v)[q] = make_int4(x[0], x[1], x[2], x[3]);
        }
    }
}

/* ---- every piece of a 128-byte record that is still in registers or LDS (instance prefixes, class chunks, with c.regs
 * the four fp32 prefixes) is stored at the END of the kernel, back to back, so that the pieces of a line meet in the L2
 * instead of reaching the memory as eight partial writes spread over the workgroup's life.  (round 4, measured and
 * removed: the records staged 64 rows at a time in LDS and stored as whole 128-byte lines, eight lanes per record -- 1.53
 * instead of 1.21 ms for the column blocks of a batch of 64: the 34 extra barriers cost more than the partial lines do;
 * the kernel is bound by its LDS / VALU work, not by its 2.15 GB of stores) */
template <int HC>
__device__ __forceinline__ void prep_store_records(const DevParams& P, const PrepLds& L, const PrepCol<HC>& c, int slow,
                                                   const InstSums& base, const PrepPlanes& pl) {
    const int H = c.H, tid = c.tid;
    if (c.regs) {
        /* The epilogue walks the column in blocks of PREP_THREADS rows, one row per thread (slot k of PrepPlanes is row
         * k * PREP_THREADS + tid), and every producer stores its pieces of the block's records before anyone goes on
         * to the next block -- no barrier, the waves only have to stay roughly together: the partial lines a workgroup
         * has in flight are 256 x 128 bytes instead of the whole column's 131 KB (x 128 workgroups per XCD: 16.8 MB
         * against 4 MB of L2 -- lines left the L2 before their last piece arrived). */
        static_assert(PREP_THREADS % 64 == 0, "a block of the epilogue: one row per thread, whole waves");
#pragma unroll
        for (int k = 0; k < c.slots; k++) {
            const int row0 = k * PREP_THREADS;
            if (row0 <= H) {
                const int v = row0 + tid;
                if (v <= H) store_gksv(c.rcol + v, pl.G[k], pl.K[k], pl.S[k], pl.V[k]);
                /* the class chunks of a wave's OWN 64 rows (the rows whose {G, K, S, V} it has just stored):
                 * lanes 0..39 = 8 blocks x 5 chunks.  Measured against a block-strided loop over the block's items:
                 * column blocks 1.04 -> 0.95 ms, fused launch 2.56 -> 2.48 ms per batch of 64 */
                const int ln = tid & 63, wv = tid >> 6;
                if (ln < 40) {
                    const int kbl = ln / 5, q = ln - kbl * 5, kb = ((row0 + 64 * wv) >> 3) + kbl;
                    if (kb * 8 <= H) prep_store_class_item(L, c, slow, kb, q);
                }
                /* (with the block that holds its first row: when R does not divide PREP_THREADS they reach into the
                 * next one) */
                if (c.r_lo >= row0 && c.r_lo < row0 + PREP_THREADS) prep_store_instance_rows(P, c, slow, base);
            }
        }
        /* (row H when it starts a block of its own -- H a multiple of PREP_THREADS: its class chunk and
         * {G, K, S, V} went out with that block above, its instance piece with row H - 1's owner) */
        return;
    }
    /* H + 1 > PREP_MAXR * PREP_THREADS rows, the prefixes are in the records already: the whole column, piece by piece */
    const int NB = (H >> 3) + 1; /* 1/8-resolution blocks; the last one holds row H only */
    for (int it = tid; it < NB * 5; it += PREP_THREADS) {
        const int kb = it / 5, q = it - kb * 5;
        prep_store_class_item(L, c, slow, kb, q);
    }
    prep_store_instance_rows(P, c, slow, base);
}

/* One column of a call: its records (RowRec), PruneRec, col_flags entry and fn windows.  The stages in order, with the
 * barriers between them and the LDS each one takes over (PrepLds).  HC > 0: compiled for a context of HC rows (PrepCol);
 * 0: the rows at run time. */
template <int HC>
__device__ __forceinline__ void prepare_columns_body(
    const DevParams& P, const int colg, char* smem, const float* __restrict__ joined,
    const int32_t* __restrict__ seg, const float* __restrict__ ground /*[img][3][H]*/,
    const int* __restrict__ vhor_arr, RowRec* __restrict__ recs, int* __restrict__ col_flags,
    float* __restrict__ sv_arr /* null: a unary call, nothing reads the copies */, PruneRec* __restrict__ prune,
    int* __restrict__ n_generic, int* __restrict__ path_bad) {
    /* the distrust word of the last call's walk: every wave of a gated k_backtrace reads it, so that launch cannot
     * clear it; the next call does, in front of its own walk */
    if (colg == 0 && threadIdx.x == 0) path_bad[0] = 0;
    if (P.lut_ready != nullptr && threadIdx.x == 0) {
        P.lut_ready[colg] = 0; /* (the fused LUT units of the DP launch count up) */
        if (colg == 0 && P.lutf_bad != nullptr) *P.lutf_bad = 0;
    }
    const PrepCol<HC> c = prep_col<HC>(P, colg, seg, recs);
    const PrepLds L = prep_lds(smem, c.NP, c.CH, c.SS);
    const int vhor = vhor_arr[c.img];
    const int H = c.H, tid = c.tid;

    prep_stage_column(P, L, c, joined); /* L.d, L.seg */
    __syncthreads();
    prep_fn_windows(P, L, c);
    InstSums base;
    const int slow = prep_instance_sums(P, L, c, col_flags, n_generic, base); /* L.wave; writes L.tot[0] */
    __syncthreads();
    const int nic_bad = prep_square_offsets(L, c); /* L.seg: the raw offsets are gone; L.wave */
    prep_class_prefixes(L, c);                     /* L.seg: prefixes */
    __syncthreads();

    PrepPlanes pl;
#pragma unroll
    for (int k = 0; k < PREP_MAXR; k++) pl.S[k] = pl.V[k] = pl.G[k] = pl.K[k] = 0.0f;
    /* compact copies for the pairwise phase 2 */
    float* svcol = sv_arr != nullptr ? sv_arr + (size_t)colg * 2 * (H + 1) : nullptr;
    prep_fill_S(P, L, c);
    prep_scan_plane(L, c, pl.S, &RowRec::S, svcol);
    __syncthreads();
    if (P.invalid >= 0) {
        prep_fill_V(P, L, c);
        prep_scan_plane(L, c, pl.V, &RowRec::V, svcol ? svcol + H + 1 : nullptr);
        __syncthreads();
    } else { /* all zero without an invalid-disparity value: no scan needed */
        for (int v = tid; v <= H; v += PREP_THREADS) {
            if (!c.regs) c.rcol[v].V = 0.0f;
            if (svcol) svcol[H + 1 + v] = 0.0f;
        }
    }
    const float2 g_red = prep_fill_G(P, L, c, ground, vhor); /* L.red */
    prep_scan_plane(L, c, pl.G, &RowRec::G, nullptr);
    __syncthreads();
    const float2 k_red = prep_fill_K(P, L, c, vhor); /* L.red */
    prep_prune_rec(P, L, c, g_red, k_red, slow, nic_bad, prune);
    prep_scan_plane(L, c, pl.K, &RowRec::K, nullptr);
    prep_store_records(P, L, c, slow, base, pl); /* no barrier: reads L.seg and registers only */
}

template <int HC>
__global__ __launch_bounds__(PREP_THREADS) void k_prepare_columns(
    const DevParams P, const float* __restrict__ joined, const int32_t* __restrict__ seg,
    const float* __restrict__ ground, const int* __restrict__ vhor_arr, RowRec* __restrict__ recs,
    int* __restrict__ col_flags, float* __restrict__ sv_arr, PruneRec* __restrict__ prune,
    int* __restrict__ n_generic, int* __restrict__ path_bad) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    prepare_columns_body<HC>(P, (int)blockIdx.x, smem, joined, seg, ground, vhor_arr, recs, col_flags, sv_arr,
                             prune, n_generic, path_bad);
}

/* ====================================================================================== */
/* A4  object data-cost prefix table (ComputeObjectLUT, StixelsKernels.cu:236-296, 959-978) */
/* ====================================================================================== */
/* lutT[v][fn] = prefix over rows of obj_cost_lut[fn][(int)d[row]] with the reference's
 * association: per 32-row block a 32-lane Kogge-Stone network (shuffle distances 1,2,4,8,16)
 * whose lane 0 first receives the running carry; blocks chained serially.
 *
 * The reference gives a warp one fn and lets lanes be rows (5 shuffles per block).  Here a LANE
 * owns one fn and evaluates the same 32-input network on registers (129 fp32 adds per block, no
 * cross-lane traffic); the 64 lanes of a wave are 64 consecutive fn, so every load of the
 * transposed cost table and every store of a lutT row is one fully coalesced 256-byte access. */
#define LUT_BLOCK 32
/* The table is 8.6 GB for a batch of 64 (1024 x 2048 x 128): its stores ARE the kernel.  Measured (batch 64,
 * the LUT units as a kernel of their own): 1.78 ms = 4.8 TB/s with plain stores; the same instruction stream
 * with the stores wrapped into 8 rows per column (absorbed by the L2) 0.48 ms; non-temporal stores (full
 * 256-byte rows that nothing reads before the whole table is written: no reason to keep them in the L2 /
 * MALL) 1.59 ms = 5.4 TB/s.  Storing fewer fn per row only pays in whole 128-byte lines (105 of 128 fn:
 * 2.37 ms, partial lines are read-modify-write). */
/*
 * CARRY (the prepare launch of a walk call, k_unary_path): only the carries, lutC[k][fn] = lutT[32 k][fn] for the
 * ceil(H / 32) blocks k of the column (lutC[0] = 0), as whole non-temporal rows of the compact [ceil(H/32)][D]
 * buffer `out` (isk_lut_carry_rows).  Only c[31] of a block is stored, so the compiler keeps the lane-31 path of the
 * network: the same additions on the same values as the full table's.  The walk rebuilds the entries it reads. */
template <bool CARRY>
__device__ __forceinline__ void object_lut_body(const DevParams& P, const int colg, const int fn_block,
                                                const int lane, const float* __restrict__ joined,
                                                const float* __restrict__ cost_T /*[dis][fn]*/,
                                                float* __restrict__ out) {
    const int H = P.H, D = P.D;
    const int fn = fn_block * 64 + lane;
    const bool fn_ok = fn < D;
    const int fnc = fn_ok ? fn : D - 1;
    const float* dcol = joined + (size_t)colg * H;
    float* lcol = out + (size_t)colg * (CARRY ? isk_lut_carry_rows(H) : H + 1) * D;
    if (fn_ok) lcol[fn] = 0.0f; /* arr[0] = 0, :283-285 (CARRY: the carry of block 0) */
    float add = 0.0f;
    /* the per-row costs of the NEXT block are fetched before this block's 32 row stores are issued:
     * a wave's memory operations retire in order, so loads queued behind the stores would wait
     * for the whole store latency */
    float cn[LUT_BLOCK];
    /* (int)d of a block's 32 rows: one coalesced load, requested a block before its costs are (a
     * wave that is alone on its SIMD -- a single frame -- otherwise waits for two dependent memory
     * round trips per block: the disparities, then the table entries they select) */
    auto fetch_d = [&](int i) -> float { return lut_row_d(dcol, i + (lane & (LUT_BLOCK - 1)), H); };
    auto fetch = [&](float d_l, float (&c)[LUT_BLOCK]) {
        const int dis_l = lut_bin(d_l, D);
#pragma unroll
        for (int l = 0; l < LUT_BLOCK; l++) { /* wave-uniform broadcasts */
            const int dis = __builtin_amdgcn_readlane(dis_l, l);
            c[l] = cost_T[(size_t)dis * D + fnc];
        }
    };
    fetch(fetch_d(0), cn);
    float d_next = fetch_d(LUT_BLOCK);
    /* One block: the next block's disparities and costs are requested, then this block's network runs
     * and its 32 rows are stored.  FULL blocks store unconditionally (lanes beyond D hold lane D - 1's
     * values and write them to its address again), so that the number of memory operations between
     * a request and its use is the same on every path and the compiler waits with a counted
     * s_waitcnt vmcnt(32) for the costs instead of vmcnt(0) for the previous block's stores as
     * well -- half of a block's time when the wave is alone on its SIMD (a single frame).  For the
     * same reason the first block is peeled: the loop is entered in its steady state. */
    auto block = [&](int i, bool full) {
        float c[LUT_BLOCK];
#pragma unroll
        for (int l = 0; l < LUT_BLOCK; l++) c[l] = cn[l];
        if (i + LUT_BLOCK < H) {
            const float d_here = d_next;
            d_next = fetch_d(i + 2 * LUT_BLOCK);
            fetch(d_here, cn);
        }
        c[0] += add; /* :249-251 */
#pragma unroll
        for (int j = 1; j < LUT_BLOCK; j <<= 1) { /* :255-263; descending l reads pre-step values */
#pragma unroll
            for (int l = LUT_BLOCK - 1; l >= j; l--) c[l] += c[l - j];
        }
        if (CARRY) {
            if (i + LUT_BLOCK < H) __builtin_nontemporal_store(c[LUT_BLOCK - 1], &lcol[(size_t)(i / LUT_BLOCK + 1) * D + fnc]);
        } else if (full) {
#pragma unroll
            for (int l = 0; l < LUT_BLOCK; l++) __builtin_nontemporal_store(c[l], &lcol[(size_t)(i + l + 1) * D + fnc]); /* :266 */
        } else if (fn_ok) {
#pragma unroll
            for (int l = 0; l < LUT_BLOCK; l++)
                if (i + l < H) lcol[(size_t)(i + l + 1) * D + fn] = c[l];
        }
        add = c[LUT_BLOCK - 1]; /* :268-272 */
    };
    int i = 0;
    if (LUT_BLOCK <= H) { /* peeled */
        block(0, true);
        i = LUT_BLOCK;
    }
    for (; i + LUT_BLOCK <= H; i += LUT_BLOCK) block(i, true);
    if (i < H) block(i, false);
}

/* The complete table by the ordinary units, behind a gate word: leaves at once while *run_if is 0 -- the normal case.
 * col_flags null: every column, else only the flagged ones.
 *  - isk_launch_lut_repair: behind a fused LUT + DP launch (k_dp_unary_fast, LUTF) whose workgroups could not trust the
 *    hand-over, or a distrusted walk: every column again;
 *  - isk_launch_lut_generic: in front of the tile launches that read the table in a walk call (k_dp_unary<.., false> for
 *    the generic-encoding columns, which the walk leaves alone): exactly those columns, gated by *n_generic. */
__global__ __launch_bounds__(64) void k_object_lut_gated(const DevParams P, int ncols, const float* __restrict__ joined,
                                                         const float* __restrict__ cost_T, float* __restrict__ lutT,
                                                         const int* __restrict__ run_if,
                                                         const int* __restrict__ col_flags) {
    if (__builtin_amdgcn_readfirstlane(*run_if) == 0) return;
    const int fn_blocks = (P.D + 63) / 64;
    for (int u = (int)blockIdx.x; u < ncols * fn_blocks; u += (int)gridDim.x) {
        const int colg = u / fn_blocks;
        if (col_flags != nullptr && __builtin_amdgcn_readfirstlane(col_flags[colg]) == 0) continue;
        object_lut_body<false>(P, colg, u - colg * fn_blocks, (int)threadIdx.x, joined, cost_T, lutT);
    }
}

/* Both preparation kernels in ONE launch: a 256-thread workgroup is either one column of
 * k_prepare_columns (blocks 0 .. ncols - 1) or four (column, 64 fn) units of object_lut_body (the
 * blocks after them).  A frame or a few: neither kernel fills the chip and both are latency chains
 * (59 + 45 us one after the other, 51 us together; on two streams they did not overlap in
 * practice).  A batch of 64: the LUT blocks start while the last column blocks drain, 2.85 instead
 * of 3.1 ms for two launches.  MEASURED alternatives: the two kinds interleaved in block order, so
 * that they share the CUs for the whole launch: 3.7 ms (and a single frame 0.349 instead of
 * 0.325 ms) -- side by side they take the memory system from each other.  (Until the LUT loop
 * stored unconditionally its body took 166 VGPRs under this kernel's launch bounds and the fused
 * launch cost a large batch the occupancy both bodies live on: 8.2 ms.) */
template <bool CARRY> /* lut: lutT, or CARRY: the walk's carry rows lutC (object_lut_body) */
__global__ __launch_bounds__(PREP_THREADS) void k_prepare_fused(
    const DevParams P, int ncols, const float* __restrict__ joined, const int32_t* __restrict__ seg,
    const float* __restrict__ ground, const int* __restrict__ vhor_arr, const float* __restrict__ cost_T,
    RowRec* __restrict__ recs, float* __restrict__ lut, int* __restrict__ col_flags,
    float* __restrict__ sv_arr, PruneRec* __restrict__ prune, int* __restrict__ n_generic,
    int* __restrict__ path_bad) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = (int)blockIdx.x;
    const bool is_lut = b >= ncols; /* the LUT blocks follow the column blocks */
    const int lut_b = b - ncols, col_b = b;
    if (is_lut) {
        const int fn_blocks = (P.D + 63) / 64;
        const int unit = lut_b * (PREP_THREADS / 64) + (int)(threadIdx.x >> 6);
        if (unit < ncols * fn_blocks)
            object_lut_body<CARRY>(P, unit / fn_blocks, unit % fn_blocks, (int)(threadIdx.x & 63), joined, cost_T, lut);
    } else {
        prepare_columns_body<0>(P, col_b, smem, joined, seg, ground, vhor_arr, recs,
                                col_flags, sv_arr, prune, n_generic, path_bad);
    }
}

/* The carry rows of a walk call from a cost table in LDS (CallPlan::lut_carry_lds; D <= 128).  object_lut_body<true>
 * loads one 256-byte piece of cost_T[dis] per row, column and 64 fn: at 16 384 columns x 1024 rows x 128 fn that is
 * 8.6 GB read through L1 / L2 out of a 64 KB table.  Here a workgroup stages the table once ([dis][NF * 64] floats;
 * the fn beyond D of a row are zero and are never stored) and then takes whole columns, one wave per column; lane l
 * owns the NF consecutive fn NF l .. NF l + NF - 1, so a row is one ds_read_b32 / ds_read_b64 per lane without bank
 * conflicts (a 32-lane half covers 64 consecutive dwords at NF = 2) and a carry row one contiguous store per wave.
 * The bins of 64 rows (two LUT blocks) come with one coalesced load, two loads ahead of their use.  Per block exactly
 * the additions that end in c[31] of object_lut_body's network, in its order on its values: l = 31, 31 - 2 j, .. of
 * step j read the lanes l - j, which that step does not write.  The block whose carry nothing reads (the last one) is
 * not evaluated. */
#define LUTC_THREADS 512
#define LUTC_MAX_WGS 512 /* two workgroups of 64 KB per CU */
typedef float lutc_f2 __attribute__((ext_vector_type(2)));
template <int NF>
__global__ __launch_bounds__(LUTC_THREADS) void k_lut_carry(const DevParams P, int ncols,
                                                            const float* __restrict__ joined,
                                                            const float* __restrict__ cost_T /*[dis][fn]*/,
                                                            float* __restrict__ lutC) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int W = NF * 64; /* floats per staged row */
    float* s_tab = reinterpret_cast<float*>(smem);
    const int H = P.H, D = P.D, nb = isk_lut_carry_rows(H);
    if ((D & 3) == 0) { /* 16-byte loads: a row of cost_T starts on a 16-byte boundary */
        for (int q = (int)threadIdx.x; q < D * (W / 4); q += LUTC_THREADS) {
            const int dis = q / (W / 4), f4 = (q - dis * (W / 4)) * 4;
            float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (f4 < D) x = *reinterpret_cast<const float4*>(cost_T + (size_t)dis * D + f4);
            *reinterpret_cast<float4*>(s_tab + dis * W + f4) = x;
        }
    } else {
        for (int q = (int)threadIdx.x; q < D * W; q += LUTC_THREADS) {
            const int dis = q / W, f = q - dis * W;
            s_tab[q] = f < D ? cost_T[(size_t)dis * D + f] : 0.0f;
        }
    }
    __syncthreads();
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int fn = NF * lane;
    const bool pair = NF == 2 && (D & 1) == 0; /* both fn of a lane on one side of D: 8-byte stores */
    for (int colg = (int)blockIdx.x * (LUTC_THREADS / 64) + wave; colg < ncols;
         colg += (int)gridDim.x * (LUTC_THREADS / 64)) {
        const float* dcol = joined + (size_t)colg * H;
        float* lcol = lutC + (size_t)colg * nb * D;
        auto store_row = [&](int k, const float (&v)[NF]) {
            float* p = lcol + (size_t)k * D + fn;
            if (pair) {
                if (fn < D) {
                    lutc_f2 x = {v[0], v[NF - 1]};
                    __builtin_nontemporal_store(x, reinterpret_cast<lutc_f2*>(p));
                }
            } else {
#pragma unroll
                for (int f = 0; f < NF; f++)
                    if (fn + f < D) __builtin_nontemporal_store(v[f], p + f);
            }
        };
        float add[NF];
#pragma unroll
        for (int f = 0; f < NF; f++) add[f] = 0.0f;
        store_row(0, add); /* arr[0] = 0, :283-285: the carry of block 0 */
        float d_here = lut_row_d(dcol, lane, H), d_next = lut_row_d(dcol, 64 + lane, H);
        for (int i0 = 0; i0 + LUT_BLOCK < H; i0 += 2 * LUT_BLOCK) {
            const int dis_l = lut_bin(d_here, D);
            d_here = d_next;
            d_next = lut_row_d(dcol, i0 + 4 * LUT_BLOCK + lane, H);
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int i = i0 + h * LUT_BLOCK;
                if (i + LUT_BLOCK < H) { /* (wave-uniform) the blocks in front of the last one */
                    float c[LUT_BLOCK][NF];
#pragma unroll
                    for (int l = 0; l < LUT_BLOCK; l++) { /* wave-uniform broadcasts */
                        const int dis = __builtin_amdgcn_readlane(dis_l, h * LUT_BLOCK + l);
                        const float* row = s_tab + dis * W + fn;
                        if (NF == 2) {
                            const lutc_f2 x = *reinterpret_cast<const lutc_f2*>(row);
                            c[l][0] = x.x;
                            c[l][NF - 1] = x.y;
                        } else {
                            c[l][0] = row[0];
                        }
                    }
#pragma unroll
                    for (int f = 0; f < NF; f++) {
                        c[0][f] += add[f]; /* :249-251 */
#pragma unroll
                        for (int j = 1; j < LUT_BLOCK; j <<= 1) {
#pragma unroll
                            for (int l = LUT_BLOCK - 1; l >= j; l -= 2 * j) c[l][f] += c[l - j][f];
                        }
                        add[f] = c[LUT_BLOCK - 1][f]; /* :268-272 */
                    }
                    store_row(i / LUT_BLOCK + 1, add);
                }
            }
        }
    }
}

/* ====================================================================================== */
/* Pairwise transition priors that depend only on vB and the frame's ground model          */
/* ====================================================================================== */
__device__ __forceinline__ float neg_fastlog_div(float v, float v2) { /* :35-38 */
    return -is_logf(v) + is_logf(v2);
}

__global__ void k_prior_tables(const DevParams P, const float* __restrict__ ground,
                               PriorRec* __restrict__ priors, int n_images) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_images * P.H) return;
    const int img = idx / P.H, vB = idx % P.H;
    const float* gfun = ground + (size_t)img * 3 * P.H;
    PriorRec r;
    r.pc = neg_fastlog_div(1.0f, (float)(P.H - vB));
    r.g_from = P.nlog03 + r.pc;
    float gprev = (vB > 0) ? gfun[vB - 1] : 0.0f;
    r.s_from_g = (gprev < 1.0f) ? r.pc : IS_INF;
    r.o_from_s = neg_fastlog_div(1.0f, P.max_disf - P.epsilon) + r.pc;
    const float base = P.nlog07 + r.pc;
    if (gprev < 0.0f) gprev = 0.0f;
    r.g_prev = gprev;
    r.og_hi = base + neg_fastlog_div(P.pgrav, P.max_disf - gprev - P.epsilon);
    r.og_lo = base + neg_fastlog_div(P.pblg, gprev - P.epsilon);
    r.og_mid = base + neg_fastlog_div(1.0f - P.pgrav - P.pblg, 2.0f * P.epsilon);
    priors[idx] = r;
}

/* k_prepare_columns of a context.  A kernel compiled for HC rows serves the contexts of HC rows: the host
 * checks that what it holds as constants -- the rows, the tree over them, the LDS carve-up -- is what DevParams and
 * isk_prepare_lds_bytes say (is_ctx_create derives P2 from the rows, so it is); any other shape takes the run-time
 * body. */
typedef void (*prep_columns_kernel_t)(const DevParams, const float*, const int32_t*, const float*, const int*, RowRec*,
                                      int*, float*, PruneRec*, int*, int*);
template <int HC>
static bool prep_compiled_for(const DevParams* P) {
    return P->H == HC && P->P2 == PrepCol<HC>::P2 && P->log2P2 == prep_log2(PrepCol<HC>::P2) &&
           prep_lds_carve_bytes(PrepCol<HC>::NP, P->CH, PrepCol<HC>::SS) == isk_prepare_lds_bytes(P);
}
static prep_columns_kernel_t prep_columns_kernel(const DevParams* P) {
    if (prep_compiled_for<1024>(P)) return k_prepare_columns<1024>;
    if (prep_compiled_for<784>(P)) return k_prepare_columns<784>;
    return k_prepare_columns<0>;
}
/* k_prepare_fused for (carry rows or the whole lutT); k_lut_carry for (D <= 64): one or two fn per lane */
static decltype(&k_prepare_fused<false>) prepare_fused_kernel(bool carry) {
    return carry ? k_prepare_fused<true> : k_prepare_fused<false>;
}
static decltype(&k_lut_carry<1>) lut_carry_kernel(bool d64) { return d64 ? k_lut_carry<1> : k_lut_carry<2>; }

extern "C" {

hipError_t isk_launch_lut_repair(const DevParams* P, int ncols, const float* joined, const float* cost_T, float* lutT,
                                 const int* run_if, hipStream_t stream) {
    const int units = ncols * ((P->D + 63) / 64);
    hipLaunchKernelGGL(k_object_lut_gated, dim3(units < 8192 ? units : 8192), dim3(64), 0, stream, *P, ncols, joined,
                       cost_T, lutT, run_if, (const int*)nullptr);
    return hipGetLastError();
}

hipError_t isk_launch_lut_generic(const DevParams* P, const CallPlan* plan, const CallBuffers* b, hipStream_t stream) {
    const int units = plan->ncols * ((P->D + 63) / 64);
    hipLaunchKernelGGL(k_object_lut_gated, dim3(units < 2048 ? units : 2048), dim3(64), 0, stream, *P, plan->ncols,
                       b->joined, b->cost_T, b->lutT, (const int*)b->n_generic, (const int*)b->col_flags);
    return hipGetLastError();
}

/* k_lut_carry serves a shape when a lane holds one or two fn (D <= 128) and the staged table leaves room for a second
 * workgroup on the CU (64 of 160 KB); 0: it does not (CallPlan::lut_carry_lds stays off) */
size_t isk_lut_carry_lds_bytes(const DevParams* P) {
    const size_t nf = ((size_t)P->D + 63) / 64, bytes = sizeof(float) * (size_t)P->D * nf * 64;
    return nf <= 2 && bytes <= 64 * 1024 ? bytes : 0;
}

hipError_t isk_launch_lut_carry(const DevParams* P, const CallPlan* plan, const CallBuffers* b, hipStream_t stream) {
    const int per_wg = LUTC_THREADS / 64, wgs = (plan->ncols + per_wg - 1) / per_wg;
    const dim3 grid(wgs < LUTC_MAX_WGS ? wgs : LUTC_MAX_WGS);
    hipLaunchKernelGGL(lut_carry_kernel(P->D <= 64), grid, dim3(LUTC_THREADS), isk_lut_carry_lds_bytes(P), stream, *P,
                       plan->ncols, b->joined, b->cost_T, b->lutC);
    return hipGetLastError();
}

/* columns one pass of k_lut_carry's grid-stride loop takes (tests: a call with more than that) */
int isk_lut_carry_pass_columns(void) { return LUTC_MAX_WGS * (LUTC_THREADS / 64); }

hipError_t isk_launch_prepare(const DevParams* P, const CallPlan* plan, const CallBuffers* b, hipStream_t stream) {
    const int ncols = plan->ncols;
    float* sv = plan->pairwise ? b->sv : nullptr; /* (only the pairwise phase 2 reads the S / V copies) */
    const bool carry_lds = plan->prepare_lut && plan->lut_carry && plan->lut_carry_lds;
    /* the records alone: the LUT units run inside the unary DP launch (k_dp_unary_fast, LUTF), or the carry rows are
     * k_lut_carry's -- both kernels only read `joined`, kernel boundaries order them in front of the DP (measured in
     * both orders: 952 + 145 and 958 + 141 us per 64 frames) */
    if (!plan->prepare_lut || carry_lds) {
        hipLaunchKernelGGL(prep_columns_kernel(P), dim3(ncols), dim3(PREP_THREADS), isk_prepare_lds_bytes(P), stream, *P,
                           b->joined, b->seg, b->ground, b->vhor, b->recs, b->col_flags, sv, b->prune, b->n_generic,
                           b->path_bad);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess || !carry_lds) return e;
        return isk_launch_lut_carry(P, plan, b, stream);
    }
    /* the two prepare kernels are independent: one launch with workgroups of both kinds (k_prepare_fused) */
    const int units = ncols * ((P->D + 63) / 64);
    const int n_lut = (units + PREP_THREADS / 64 - 1) / (PREP_THREADS / 64);
    hipLaunchKernelGGL(prepare_fused_kernel(plan->lut_carry != 0), dim3(ncols + n_lut), dim3(PREP_THREADS),
                       isk_prepare_lds_bytes(P), stream, *P, ncols, b->joined, b->seg, b->ground, b->vhor, b->cost_T, b->recs,
                       plan->lut_carry ? b->lutC : b->lutT, b->col_flags, sv, b->prune, b->n_generic, b->path_bad);
    return hipGetLastError();
}

hipError_t isk_launch_priors(const DevParams* P, const float* ground, PriorRec* priors,
                             int n_images, hipStream_t stream) {
    const int n = n_images * P->H;
    hipLaunchKernelGGL(k_prior_tables, dim3((n + 255) / 256), dim3(256), 0, stream, *P, ground,
                       priors, n_images);
    return hipGetLastError();
}

hipError_t isk_set_lds_prepare(const DevParams* P) {
    const void* kernels[3] = {(const void*)prep_columns_kernel(P), (const void*)prepare_fused_kernel(false),
                              (const void*)prepare_fused_kernel(true)};
    for (const void* k : kernels) {
        const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)isk_prepare_lds_bytes(P));
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t isk_set_lds_lut_carry(const DevParams* P) {
    const int bytes = (int)isk_lut_carry_lds_bytes(P);
    if (bytes == 0) return hipSuccess; /* the shape keeps k_prepare_fused<true> */
    return hipFuncSetAttribute((const void*)lut_carry_kernel(P->D <= 64), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

} /* extern "C" */
