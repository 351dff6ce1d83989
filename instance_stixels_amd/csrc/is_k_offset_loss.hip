/*
 * is_k_offset_loss.hip -- f12: the two "SL" regression losses of the reference's CNN training for a batch, with the
 * gradient with respect to the prediction (is_offset_loss of instance_stixels_core.h).  It replaces the Python loops
 * per frame and per instance id of tools/CNN_training/losses.py (OffsetLossSL :127-175, DisparityOffsetLossSL :24-125)
 * and the autograd replay behind them.  The numpy restatement is tests/offset_loss_reference.py.
 *
 * Every sum over predictions is binary64 and is combined in an order that the input alone decides; there is no
 * floating-point atomic.  A frame's cells are cut into chunks of 64 adjacent cells (image order, across row ends) and
 * its chunks into at most OL_PARTS partitions of adjacent chunks.  A partition is one wave and owns one slice
 * [capacity + 1][sums] of the partial tables: per chunk it takes the key of the first unfinished lane, reduces the
 * masked values of the lanes that hold it with a fixed butterfly, adds the totals to the key's row of its slice with
 * plain loads and stores (one lane per column, so each address has one writer), and repeats until every lane is done.
 * A reducer, one wave per key, then adds the partitions' rows, a lane per partition, with the same butterfly.  Stuff
 * is row `capacity`.  The rows are the keys' RANKS (the number of keys of the frame below it), not their numbers of
 * arrival, so the order of the final sum over the keys does not depend on the arrival either.  On the caller's
 * stream, behind one memset:
 *
 *   k_ol_keys      one lane per cell: the first lane of a run of equal keys enters the key into the frame's table
 *                  (is_gt_keys.h) and notes the slot under the key's number of arrival;
 *   k_ol_rank      the keys' ranks; the key counts; on overflow NaN into d_loss and d_terms, and every later launch
 *                  returns at once;
 *   k_ol_sums      pass 1 per partition: n, sum y, sum x (integers), sum pos_y, sum pos_x, sum disp; the cells' q into
 *                  [rank][256] histograms (integer atomics);
 *   k_ol_stats     one wave per row: g, m, md and the lower median of the histogram;
 *   k_ol_spread    pass 2 per partition: sum |pos - g|, sum (pos - m)^2 or sum |pos - m| with the sums of the signs,
 *                  sum |disp - med|, sum (disp - md)^2 or its abs form; for stuff sum |off| and sum |disp|;
 *   k_ol_parts     one wave per row: the row's contribution to the frame's four terms, the mean signs;
 *   k_ol_terms     one workgroup per frame: the four terms, keys in ascending rank, then stuff;
 *   k_ol_loss      one workgroup: the batch sums and the weighted loss;
 *   k_ol_grad      one lane per cell: the gradient of all planes, zeros included.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "instance_stixels_core.h"
#include "is_gt_keys.h"
#include "is_launch.h"

#define OL_THREADS 256
#define OL_WAVES (OL_THREADS / 64)
#define OL_PARTS 64 /* partitions of a frame at most: a lane of the reducers each */
#define OL_S2 8     /* columns of a pass-2 row: A, V, SY, SX, D, DV, SD, (pad) */
#define OL_STAT 10  /* columns of a row's statistics */
enum { ST_N, ST_GY, ST_GX, ST_MY, ST_MX, ST_MD, ST_MED, ST_SY, ST_SX, ST_SD };

struct OlLayout {
    size_t overflow, count, table, hist, part_i, part1, part2, zero_end, slot, stat, contrib, terms, total;
};

struct OlArgs {
    int* overflow;              /* [4]: word 0 != 0: a frame has more keys than rows */
    int32_t* count;             /* [n] keys per frame */
    GttEntry* table;            /* [n][slots] */
    unsigned* hist;             /* [n][capacity][GTT_BINS] by rank (3 planes) */
    unsigned long long* part_i; /* [n][parts][capacity + 1][3]: n, sum y, sum x */
    double* part1;              /* [n][parts][capacity + 1][3]: sum pos_y, sum pos_x, sum disp */
    double* part2;              /* [n][parts][capacity + 1][OL_S2] */
    int32_t* slot;              /* [n][capacity]: the table slot of the key with that number of arrival */
    double* stat;               /* [n][capacity + 1][OL_STAT] */
    double* contrib;            /* [n][capacity + 1][4] */
    double* terms;              /* [n][4] */
    const float* pred;
    long long pred_stride;
    const int32_t* ids;
    const uint16_t* disp8;
    int n, planes, Hs, Ws, capacity, abs_variance;
    unsigned log_slots;
    int chunks, parts, cpp; /* chunks of a frame, its partitions, chunks per partition */
    double w_om, w_ov, w_dm, w_dv;
    float* loss;
    float* out_terms;
    float* grad;
    long long grad_stride;
    int32_t* key_count;
};

static void ol_partition(size_t cells, int& chunks, int& parts, int& cpp) {
    chunks = (int)((cells + 63) / 64);
    cpp = (chunks + OL_PARTS - 1) / OL_PARTS;
    parts = (chunks + cpp - 1) / cpp;
}

static OlLayout ol_layout(size_t n, size_t cells, int planes, size_t capacity) {
    OlLayout l;
    size_t o = 0;
    auto take = [&o](size_t bytes) {
        const size_t at = o;
        o += (bytes + 15) & ~(size_t)15;
        return at;
    };
    int chunks, parts, cpp;
    ol_partition(cells, chunks, parts, cpp);
    const size_t rows = n * (size_t)parts * (capacity + 1);
    l.overflow = take(4 * sizeof(int));
    l.count = take(n * sizeof(int32_t));
    l.table = take(n * ((size_t)1 << gtt_log_slots(cells)) * sizeof(GttEntry));
    l.hist = take(planes == 3 ? n * capacity * GTT_BINS * sizeof(unsigned) : 0);
    l.part_i = take(rows * 3 * sizeof(unsigned long long));
    l.part1 = take(rows * 3 * sizeof(double));
    l.part2 = take(rows * OL_S2 * sizeof(double));
    l.zero_end = o; /* [0, zero_end) is cleared in front of every call */
    l.slot = take(n * capacity * sizeof(int32_t));
    l.stat = take(n * (capacity + 1) * OL_STAT * sizeof(double));
    l.contrib = take(n * (capacity + 1) * 4 * sizeof(double));
    l.terms = take(n * 4 * sizeof(double));
    l.total = o;
    return l;
}

/* torch's sign: 0 at 0 */
__device__ __forceinline__ double ol_sign(double v) { return (double)((v > 0.0) - (v < 0.0)); }

/* The row of a cell: its key's rank, `capacity` for stuff (id < 11 or id == 255), -1 for a cell that contributes
 * nothing. */
__device__ __forceinline__ int ol_row(const OlArgs& a, const GttEntry* table, int id) {
    if (id > 1000) {
        const GttEntry* e = gtt_find(table, a.log_slots, id);
        return e ? e->rank : -1;
    }
    return (id < 11 || id == 255) ? a.capacity : -1;
}

/* the total over the wave in every lane: a fixed butterfly, lanes that do not take part hold 0 */
template <class T> __device__ __forceinline__ T ol_wave_sum(T v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

/* (frame, partition) of this wave; false: none */
__device__ __forceinline__ bool ol_part(const OlArgs& a, int& f, int& b) {
    const long long w = (long long)blockIdx.x * OL_WAVES + (threadIdx.x >> 6);
    if (w >= (long long)a.n * a.parts) return false;
    f = (int)(w / a.parts);
    b = (int)(w % a.parts);
    return true;
}

__global__ __launch_bounds__(OL_THREADS) void k_ol_keys(const OlArgs a) {
    const size_t cells = (size_t)a.Hs * a.Ws;
    const size_t cell = (size_t)blockIdx.x * OL_THREADS + threadIdx.x; /* (a wave's 64 cells are one chunk) */
    const int f = blockIdx.y, lane = threadIdx.x & 63;
    int key = 0;
    if (cell < cells) {
        const int id = a.ids[(size_t)f * cells + cell];
        if (id > 1000) key = id;
    }
    const int before = __shfl_up(key, 1, 64);
    int next;
    if (!gtt_run_head(key != before, key != 0, lane, next)) return;
    int fresh;
    const unsigned at = gtt_enter(a.table + ((size_t)f << a.log_slots), a.log_slots, key, &a.count[f], fresh);
    if (fresh >= a.capacity) a.overflow[0] = 1;
    else if (fresh >= 0) a.slot[(size_t)f * a.capacity + fresh] = (int32_t)at;
}

/* grid (ceil(capacity / OL_THREADS), n) */
__global__ __launch_bounds__(OL_THREADS) void k_ol_rank(const OlArgs a) {
    __shared__ int s_key[OL_THREADS];
    const int f = blockIdx.y, count = a.count[f];
    if (a.key_count && blockIdx.x == 0 && threadIdx.x == 0) a.key_count[f] = count;
    if (a.overflow[0]) { /* (the whole grid alike) */
        if (blockIdx.x == 0 && a.out_terms && threadIdx.x < 4) a.out_terms[(size_t)f * 4 + threadIdx.x] = NAN;
        if (blockIdx.x == 0 && f == 0 && threadIdx.x < 5) a.loss[threadIdx.x] = NAN;
        return;
    }
    if ((int)(blockIdx.x * OL_THREADS) >= count) return; /* (whole workgroups) */
    GttEntry* const table = a.table + ((size_t)f << a.log_slots);
    const int32_t* const slot = a.slot + (size_t)f * a.capacity;
    const int i = blockIdx.x * OL_THREADS + threadIdx.x;
    const int mine = i < count ? table[slot[i]].key : 0;
    int rank = 0;
    for (int base = 0; base < count; base += OL_THREADS) {
        const int j = base + threadIdx.x;
        __syncthreads();
        s_key[threadIdx.x] = j < count ? table[slot[j]].key : 0x7fffffff;
        __syncthreads();
        const int m = min(OL_THREADS, count - base);
        for (int t = 0; t < m; t++) rank += s_key[t] < mine;
    }
    if (i < count) table[slot[i]].rank = rank;
}

/* pass 1 */
__global__ __launch_bounds__(OL_THREADS) void k_ol_sums(const OlArgs a) {
    if (a.overflow[0]) return;
    int f, b;
    if (!ol_part(a, f, b)) return; /* (whole waves) */
    const int lane = threadIdx.x & 63;
    const size_t cells = (size_t)a.Hs * a.Ws;
    const GttEntry* const table = a.table + ((size_t)f << a.log_slots);
    const int32_t* const ids = a.ids + (size_t)f * cells;
    const float* const P = a.pred + (long long)f * a.pred_stride;
    const float* const Py = P + (a.planes == 3 ? cells : 0);
    const float* const Px = Py + cells;
    const size_t slice = ((size_t)f * a.parts + b) * (size_t)(a.capacity + 1);
    const int c_end = min((b + 1) * a.cpp, a.chunks);
    for (int c = b * a.cpp; c < c_end; c++) {
        const size_t cell = (size_t)c * 64 + lane;
        int row = -1;
        unsigned long long y = 0, x = 0;
        double py = 0.0, px = 0.0, d = 0.0;
        if (cell < cells) {
            row = ol_row(a, table, ids[cell]);
            if (row >= 0) {
                y = cell / (size_t)a.Ws;
                x = cell % (size_t)a.Ws;
                py = (double)Py[cell] + (double)y;
                px = (double)Px[cell] + (double)x;
                if (a.planes == 3) {
                    d = (double)P[cell];
                    const unsigned q = (unsigned)a.disp8[(size_t)f * cells + cell] >> 8;
                    if (row < a.capacity && q != 0) /* a zero is not part of any median */
                        atomicAdd(&a.hist[((size_t)f * a.capacity + row) * GTT_BINS + q], 1u);
                }
            }
        }
        uint64_t todo = __ballot(row >= 0);
        while (todo) {
            const int k = __shfl(row, __builtin_ctzll(todo), 64);
            const bool mine = row == k;
            const uint64_t members = __ballot(mine);
            todo &= ~members;
            const unsigned long long ty = ol_wave_sum(mine ? y : 0ull), tx = ol_wave_sum(mine ? x : 0ull);
            const double tpy = ol_wave_sum(mine ? py : 0.0), tpx = ol_wave_sum(mine ? px : 0.0),
                         td = ol_wave_sum(mine ? d : 0.0);
            const size_t at = (slice + (size_t)k) * 3;
            if (lane < 3)
                a.part_i[at + lane] += lane == 0 ? (unsigned long long)__popcll(members) : lane == 1 ? ty : tx;
            else if (lane < 6)
                a.part1[at + lane - 3] += lane == 3 ? tpy : lane == 4 ? tpx : td;
        }
    }
}

/* grid (ceil((capacity + 1) / OL_WAVES), n): one wave per row.  False: the row is not in use. */
__device__ __forceinline__ bool ol_reducer_row(const OlArgs& a, int& f, int& row) {
    f = blockIdx.y;
    row = blockIdx.x * OL_WAVES + (threadIdx.x >> 6);
    return row == a.capacity || row < a.count[f];
}

__global__ __launch_bounds__(OL_THREADS) void k_ol_stats(const OlArgs a) {
    if (a.overflow[0]) return;
    int f, row;
    if (!ol_reducer_row(a, f, row)) return; /* (whole waves) */
    const int lane = threadIdx.x & 63;
    const size_t stride = (size_t)(a.capacity + 1) * 3;
    const size_t first = ((size_t)f * a.parts * (a.capacity + 1) + row) * 3;
    /* lane b holds partition b (parts <= 64 = OL_PARTS): one round of loads, then the butterfly */
    unsigned long long iv[3] = {0, 0, 0};
    double dv[3] = {0.0, 0.0, 0.0};
    if (lane < a.parts) {
#pragma unroll
        for (int s = 0; s < 3; s++) {
            iv[s] = a.part_i[first + lane * stride + s];
            dv[s] = a.part1[first + lane * stride + s];
        }
    }
    const double n = (double)ol_wave_sum(iv[0]), sy = (double)ol_wave_sum(iv[1]), sx = (double)ol_wave_sum(iv[2]);
    const double spy = ol_wave_sum(dv[0]), spx = ol_wave_sum(dv[1]), sd = ol_wave_sum(dv[2]);
    double med = -1.0; /* none */
    if (a.planes == 3 && row < a.capacity) {
        unsigned N;
        const int bin = gtt_lower_median(a.hist + ((size_t)f * a.capacity + row) * GTT_BINS, lane, N);
        if (N) med = (double)bin;
    }
    if (lane != 0) return;
    double* st = a.stat + ((size_t)f * (a.capacity + 1) + row) * OL_STAT;
    st[ST_N] = n;
    st[ST_GY] = sy / n;
    st[ST_GX] = sx / n;
    st[ST_MY] = spy / n;
    st[ST_MX] = spx / n;
    st[ST_MD] = sd / n;
    st[ST_MED] = med;
}

/* pass 2 */
__global__ __launch_bounds__(OL_THREADS) void k_ol_spread(const OlArgs a) {
    if (a.overflow[0]) return;
    int f, b;
    if (!ol_part(a, f, b)) return; /* (whole waves) */
    const int lane = threadIdx.x & 63;
    const size_t cells = (size_t)a.Hs * a.Ws;
    const GttEntry* const table = a.table + ((size_t)f << a.log_slots);
    const int32_t* const ids = a.ids + (size_t)f * cells;
    const float* const P = a.pred + (long long)f * a.pred_stride;
    const float* const Py = P + (a.planes == 3 ? cells : 0);
    const float* const Px = Py + cells;
    const size_t slice = ((size_t)f * a.parts + b) * (size_t)(a.capacity + 1);
    const int c_end = min((b + 1) * a.cpp, a.chunks);
    for (int c = b * a.cpp; c < c_end; c++) {
        const size_t cell = (size_t)c * 64 + lane;
        int row = -1;
        double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; /* A, V, SY, SX, D, DV, SD */
        if (cell < cells) {
            row = ol_row(a, table, ids[cell]);
            if (row >= 0) {
                const double oy = (double)Py[cell], ox = (double)Px[cell], d = a.planes == 3 ? (double)P[cell] : 0.0;
                if (row == a.capacity) {
                    v[0] = fabs(oy) + fabs(ox);
                    v[4] = fabs(d);
                } else {
                    const double* st = a.stat + ((size_t)f * (a.capacity + 1) + row) * OL_STAT;
                    const double py = oy + (double)(cell / (size_t)a.Ws), px = ox + (double)(cell % (size_t)a.Ws);
                    const double ey = py - st[ST_MY], ex = px - st[ST_MX], ed = d - st[ST_MD];
                    v[0] = fabs(py - st[ST_GY]) + fabs(px - st[ST_GX]);
                    if (a.abs_variance) {
                        v[1] = fabs(ey) + fabs(ex);
                        v[2] = ol_sign(ey);
                        v[3] = ol_sign(ex);
                        v[5] = fabs(ed);
                        v[6] = ol_sign(ed);
                    } else {
                        v[1] = ey * ey + ex * ex;
                        v[5] = ed * ed;
                    }
                    if (st[ST_MED] >= 0.0) v[4] = fabs(d - st[ST_MED]);
                }
            }
        }
        uint64_t todo = __ballot(row >= 0);
        while (todo) {
            const int k = __shfl(row, __builtin_ctzll(todo), 64);
            const bool mine = row == k;
            todo &= ~__ballot(mine);
            double put = 0.0;
#pragma unroll
            for (int s = 0; s < 7; s++) {
                const double t = ol_wave_sum(mine ? v[s] : 0.0);
                if (lane == s) put = t;
            }
            if (lane < 7) a.part2[(slice + (size_t)k) * OL_S2 + lane] += put;
        }
    }
}

__global__ __launch_bounds__(OL_THREADS) void k_ol_parts(const OlArgs a) {
    if (a.overflow[0]) return;
    int f, row;
    if (!ol_reducer_row(a, f, row)) return; /* (whole waves) */
    const int lane = threadIdx.x & 63;
    const size_t stride = (size_t)(a.capacity + 1) * OL_S2;
    const size_t first = ((size_t)f * a.parts * (a.capacity + 1) + row) * OL_S2;
    double t[7];
#pragma unroll
    for (int s = 0; s < 7; s++) t[s] = ol_wave_sum(lane < a.parts ? a.part2[first + lane * stride + s] : 0.0);
    const double A = t[0], V = t[1], SY = t[2], SX = t[3], D = t[4], DV = t[5], SD = t[6];
    if (lane != 0) return;
    double* st = a.stat + ((size_t)f * (a.capacity + 1) + row) * OL_STAT;
    double* c = a.contrib + ((size_t)f * (a.capacity + 1) + row) * 4;
    const double n = st[ST_N];
    c[0] = A / n / 2.0; /* stuff without a cell: 0 / 0, as the reference */
    if (row == a.capacity) {
        c[1] = 0.0;
        c[2] = a.planes == 3 ? D / n : 0.0;
        c[3] = 0.0;
        return;
    }
    const bool spread = !a.abs_variance || n > 2.0;
    c[1] = spread ? V / n / 2.0 : 0.0;
    c[2] = st[ST_MED] >= 0.0 ? D / n : 0.0;
    c[3] = spread && a.planes == 3 ? DV / n : 0.0;
    st[ST_SY] = SY / n;
    st[ST_SX] = SX / n;
    st[ST_SD] = SD / n;
}

/* The sum of the workgroup's values in thread 0, by a fixed tree. */
__device__ __forceinline__ double ol_block_sum(double v, double* s) {
    __syncthreads();
    s[threadIdx.x] = v;
    __syncthreads();
    for (int o = OL_THREADS / 2; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    return s[0];
}

/* grid n */
__global__ __launch_bounds__(OL_THREADS) void k_ol_terms(const OlArgs a) {
    __shared__ double s[OL_THREADS];
    if (a.overflow[0]) return;
    const int f = blockIdx.x, count = a.count[f];
    const double* c = a.contrib + (size_t)f * (a.capacity + 1) * 4;
    for (int t = 0; t < 4; t++) {
        double v = 0.0;
        for (int row = threadIdx.x; row < count; row += OL_THREADS) v += c[(size_t)row * 4 + t];
        const double keys = ol_block_sum(v, s);
        if (threadIdx.x == 0) {
            const double term = keys + c[(size_t)a.capacity * 4 + t];
            a.terms[(size_t)f * 4 + t] = term;
            if (a.out_terms) a.out_terms[(size_t)f * 4 + t] = (float)term;
        }
    }
}

/* grid 1 */
__global__ __launch_bounds__(OL_THREADS) void k_ol_loss(const OlArgs a) {
    __shared__ double s[OL_THREADS];
    if (a.overflow[0]) return;
    double sum[4];
    for (int t = 0; t < 4; t++) {
        double v = 0.0;
        for (int f = threadIdx.x; f < a.n; f += OL_THREADS) v += a.terms[(size_t)f * 4 + t];
        sum[t] = ol_block_sum(v, s);
    }
    if (threadIdx.x != 0) return;
    double loss = a.w_om * sum[0] + a.w_ov * sum[1];
    if (a.planes == 3) loss = loss + a.w_dm * sum[2] + a.w_dv * sum[3];
    a.loss[0] = (float)loss;
    for (int t = 0; t < 4; t++) a.loss[1 + t] = (float)sum[t];
}

/* grid (ceil(cells / OL_THREADS), n) */
__global__ __launch_bounds__(OL_THREADS) void k_ol_grad(const OlArgs a) {
    if (a.overflow[0]) return;
    const size_t cells = (size_t)a.Hs * a.Ws;
    const size_t cell = (size_t)blockIdx.x * OL_THREADS + threadIdx.x;
    if (cell >= cells) return;
    const int f = blockIdx.y;
    const float* const P = a.pred + (long long)f * a.pred_stride;
    const float* const Py = P + (a.planes == 3 ? cells : 0);
    const float* const Px = Py + cells;
    const int row = ol_row(a, a.table + ((size_t)f << a.log_slots), a.ids[(size_t)f * cells + cell]);
    double gy = 0.0, gx = 0.0, gd = 0.0;
    if (row >= 0) {
        const double* st = a.stat + ((size_t)f * (a.capacity + 1) + row) * OL_STAT;
        const double n = st[ST_N];
        const double oy = (double)Py[cell], ox = (double)Px[cell], d = a.planes == 3 ? (double)P[cell] : 0.0;
        if (row == a.capacity) {
            if (a.w_om != 0.0) {
                gy = a.w_om * (ol_sign(oy) / (2.0 * n));
                gx = a.w_om * (ol_sign(ox) / (2.0 * n));
            }
            if (a.w_dm != 0.0) gd = a.w_dm * (ol_sign(d) / n);
        } else {
            const double py = oy + (double)(cell / (size_t)a.Ws), px = ox + (double)(cell % (size_t)a.Ws);
            const double ey = py - st[ST_MY], ex = px - st[ST_MX], ed = d - st[ST_MD];
            if (a.w_om != 0.0) {
                gy = a.w_om * (ol_sign(py - st[ST_GY]) / (2.0 * n));
                gx = a.w_om * (ol_sign(px - st[ST_GX]) / (2.0 * n));
            }
            if (a.w_dm != 0.0 && st[ST_MED] >= 0.0) gd = a.w_dm * (ol_sign(d - st[ST_MED]) / n);
            if (!a.abs_variance) {
                if (a.w_ov != 0.0) {
                    gy += a.w_ov * (ey / n);
                    gx += a.w_ov * (ex / n);
                }
                if (a.w_dv != 0.0) gd += a.w_dv * (2.0 * ed / n);
            } else if (n > 2.0) {
                if (a.w_ov != 0.0) {
                    gy += a.w_ov * ((ol_sign(ey) - st[ST_SY]) / (2.0 * n));
                    gx += a.w_ov * ((ol_sign(ex) - st[ST_SX]) / (2.0 * n));
                }
                if (a.w_dv != 0.0) gd += a.w_dv * ((ol_sign(ed) - st[ST_SD]) / n);
            }
        }
    }
    float* g = a.grad + (long long)f * a.grad_stride + cell;
    if (a.planes == 3) {
        g[0] = (float)gd;
        g += cells;
    }
    g[0] = (float)gy;
    g[cells] = (float)gx;
}

extern "C" {

size_t isk_offset_loss_scratch_bytes(int n_images, int planes, int Hs, int Ws, int capacity) {
    return ol_layout((size_t)n_images, (size_t)Hs * Ws, planes, (size_t)capacity).total;
}

/* The arguments are checked by is_offset_loss; capacity is the effective one. */
hipError_t isk_launch_offset_loss(const is_offset_loss_args* r, int capacity, hipStream_t stream) {
    const size_t n = (size_t)r->n_images, cells = (size_t)r->rows8 * r->cols8;
    const OlLayout l = ol_layout(n, cells, r->planes, (size_t)capacity);
    char* const base = (char*)r->d_scratch;
    OlArgs a = {};
    a.overflow = (int*)(base + l.overflow);
    a.count = (int32_t*)(base + l.count);
    a.table = (GttEntry*)(base + l.table);
    a.hist = (unsigned*)(base + l.hist);
    a.part_i = (unsigned long long*)(base + l.part_i);
    a.part1 = (double*)(base + l.part1);
    a.part2 = (double*)(base + l.part2);
    a.slot = (int32_t*)(base + l.slot);
    a.stat = (double*)(base + l.stat);
    a.contrib = (double*)(base + l.contrib);
    a.terms = (double*)(base + l.terms);
    a.pred = r->d_prediction;
    a.pred_stride = r->prediction_image_stride;
    a.ids = r->d_ids8;
    a.disp8 = r->d_disparity8_u16;
    a.n = r->n_images;
    a.planes = r->planes;
    a.Hs = r->rows8;
    a.Ws = r->cols8;
    a.capacity = capacity;
    a.abs_variance = r->abs_variance != 0;
    a.log_slots = gtt_log_slots(cells);
    ol_partition(cells, a.chunks, a.parts, a.cpp);
    a.w_om = (double)r->w_offset_mean;
    a.w_ov = (double)r->w_offset_variance;
    a.w_dm = r->planes == 3 ? (double)r->w_disparity_mean : 0.0;
    a.w_dv = r->planes == 3 ? (double)r->w_disparity_variance : 0.0;
    a.loss = r->d_loss;
    a.out_terms = r->d_terms;
    a.grad = r->d_grad;
    a.grad_stride = r->grad_image_stride;
    a.key_count = r->d_key_count;
    hipError_t e = hipMemsetAsync(base, 0, l.zero_end, stream);
    if (e != hipSuccess) return e;
    const dim3 threads(OL_THREADS);
    const dim3 cell_grid((unsigned)((cells + OL_THREADS - 1) / OL_THREADS), (unsigned)n);
    const dim3 part_grid((unsigned)((n * a.parts + OL_WAVES - 1) / OL_WAVES));
    const dim3 row_grid((unsigned)((capacity + 1 + OL_WAVES - 1) / OL_WAVES), (unsigned)n);
    hipLaunchKernelGGL(k_ol_keys, cell_grid, threads, 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_ol_rank, dim3((unsigned)((capacity + OL_THREADS - 1) / OL_THREADS), (unsigned)n), threads, 0,
                       stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_ol_sums, part_grid, threads, 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_ol_stats, row_grid, threads, 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_ol_spread, part_grid, threads, 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_ol_parts, row_grid, threads, 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_ol_terms, dim3((unsigned)n), threads, 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_ol_loss, dim3(1), threads, 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (r->d_grad) {
        hipLaunchKernelGGL(k_ol_grad, cell_grid, threads, 0, stream, a);
        e = hipGetLastError();
    }
    return e;
}

} /* extern "C" */
