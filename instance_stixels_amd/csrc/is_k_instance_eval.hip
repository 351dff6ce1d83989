/*
 * is_k_instance_eval.hip -- f6: the joint histogram of each frame's stixel instance image and its ground-truth
 * instanceIds, as a sorted sparse table (is_instance_overlap of instance_stixels_core.h).  The host turns the
 * tables of a validation set into the Cityscapes instance AP (evaluation.CityscapesInstanceEval); the numpy
 * restatement is tests/instance_eval_reference.py.
 *
 * k_iov takes is_k_render's layout: one lane owns one stixel column and IS_IOV_RCH rows, the 64 lanes of a wave
 * are 64 adjacent columns, 4 waves stack vertically.  The lane paints the covering section of each of its rows
 * into an LDS strip (highest section index wins, as the render), so the instance image is never materialised:
 * it reads 4 B per pixel of ground truth and the Sections.  Runs of equal (pred, gt) -- along a row and down the
 * rows -- are tallied in registers; each run goes into an LDS hash of 64-bit keys (linear probing, CAS on the
 * key, add on the count).  A run that finds no slot within IS_IOV_LDS_PROBES probes goes straight to the
 * frame's global hash; at the end the workgroup flushes its non-empty LDS slots there with device-scope atomics
 * (one insert per distinct pair per workgroup: a few hundred per 64K pixels, spread over the hash).
 *
 * Key: ((pred ^ 0x80000000) << 32) | (gt ^ 0x80000000), so the unsigned order of keys is the signed order of
 * (pred, gt).  The all-ones key is the empty slot; the one pair it encodes (pred = gt = INT32_MAX, reachable only
 * with hostile classes and gt) is counted in a per-frame counter of its own and emitted last.
 *
 * The global hash of a frame has 2P slots, P = the power of two >= capacity.  Every new key bumps the frame's
 * distinct counter; past the capacity the frame's flag is set and later inserts into that frame return at once,
 * so hostile gt (a new pair per pixel) costs one flag load per run, never a long probe.  The finalize gathers
 * the keys into [n][P] (padded with all-ones), bitonic-sorts them -- in LDS for blocks of IS_IOV_SORT_LDS keys,
 * with global merge steps above (k_road_sort is the one-block form) -- and emits the records, each count looked
 * up in the hash.  All counts are integers and the order is fixed: the same bytes on every run.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "instance_stixels_core.h"
#include "is_launch.h"

#define IS_IOV_RCH 32          /* image rows per lane */
#define IS_IOV_WAVES 4         /* waves per workgroup: 128 rows x 64 stixel columns */
#define IS_IOV_LDS_SLOTS 2048  /* LDS hash: 16 KiB of keys + 8 KiB of counts (+ 16 KiB strip: 40 KiB per WG) */
#define IS_IOV_LDS_PROBES 32
#define IS_IOV_SORT_LDS 4096   /* keys per LDS sort block (32 KiB) */
#define IS_IOV_SORT_THREADS 1024

typedef unsigned long long u64;
#define IOV_EMPTY (~0ull)

/* per-frame counters of the scratch */
enum { IOV_DISTINCT = 0, IOV_SENTINEL, IOV_FLAG, IOV_FILL, IOV_NCNT };

struct IovArgs {
    const is_section* sections;
    const int32_t* section_instance;
    const int32_t* gt;
    u64* gkeys;             /* [n][2P] */
    unsigned* gcnt;         /* [n][2P] */
    int* fc;                /* [n][IOV_NCNT] */
    int realcols, max_sections, rows, cols, w, xlanes, row_groups, capacity, slots_log2;
};

__device__ __forceinline__ u64 iov_key(int32_t p, int32_t g) {
    return ((u64)((uint32_t)p ^ 0x80000000u) << 32) | (u64)((uint32_t)g ^ 0x80000000u);
}

__device__ __forceinline__ unsigned iov_hash(u64 k, int log2) {
    return (unsigned)((k * 0x9E3779B97F4A7C15ull) >> (64 - log2));
}

/* The frame's global hash: add n to key's slot (a new key takes an empty one).  Past the capacity the frame is
 * flagged and the insert dropped; a flagged frame drops every later insert. */
__device__ void iov_global_insert(const IovArgs& a, int f, u64 key, unsigned n) {
    int* fc = a.fc + (size_t)f * IOV_NCNT;
    if (key == IOV_EMPTY) {
        atomicAdd((unsigned*)&fc[IOV_SENTINEL], n);
        return;
    }
    if (__hip_atomic_load(&fc[IOV_FLAG], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    const unsigned slots = 1u << a.slots_log2;
    u64* keys = a.gkeys + ((size_t)f << a.slots_log2);
    unsigned* cnt = a.gcnt + ((size_t)f << a.slots_log2);
    unsigned s = iov_hash(key, a.slots_log2);
    for (unsigned i = 0; i < slots; i++, s = (s + 1) & (slots - 1)) {
        const u64 old = atomicCAS(&keys[s], IOV_EMPTY, key);
        if (old == IOV_EMPTY) {
            if (atomicAdd(&fc[IOV_DISTINCT], 1) >= a.capacity) {
                atomicExch(&fc[IOV_FLAG], 1);
                return;
            }
            atomicAdd(&cnt[s], n);
            return;
        }
        if (old == key) {
            atomicAdd(&cnt[s], n);
            return;
        }
    }
    atomicExch(&fc[IOV_FLAG], 1);
}

__device__ __forceinline__ void iov_flush(const IovArgs& a, int f, u64* lkeys, unsigned* lcnt, u64 key,
                                          unsigned n) {
    if (key != IOV_EMPTY) {
        unsigned s = iov_hash(key, 11) & (IS_IOV_LDS_SLOTS - 1);
        for (int i = 0; i < IS_IOV_LDS_PROBES; i++, s = (s + 1) & (IS_IOV_LDS_SLOTS - 1)) {
            const u64 old = atomicCAS(&lkeys[s], IOV_EMPTY, key);
            if (old == IOV_EMPTY || old == key) {
                atomicAdd(&lcnt[s], n);
                return;
            }
        }
    }
    iov_global_insert(a, f, key, n);
}

#define IOV_TALLY(K)                                           \
    do {                                                       \
        const u64 k__ = (K);                                   \
        if (k__ == run_key) {                                  \
            run++;                                             \
        } else {                                               \
            if (run) iov_flush(a, f, lkeys, lcnt, run_key, run); \
            run_key = k__;                                     \
            run = 1;                                           \
        }                                                      \
    } while (0)

static_assert(IS_IOV_LDS_SLOTS == 1 << 11, "iov_flush hashes into 2^11 LDS slots");

/* VEC: w == 8, cols % 8 == 0 and a 16-byte aligned gt: two 16-B loads per row for the stixel columns; the tail
 * lane (pixels right of realcols * w) always takes the per-pixel path. */
template <bool VEC>
__global__ __launch_bounds__(64 * IS_IOV_WAVES) void k_iov(const IovArgs a) {
    __shared__ int16_t strip[IS_IOV_WAVES][IS_IOV_RCH][64];
    __shared__ u64 lkeys[IS_IOV_LDS_SLOTS];
    __shared__ unsigned lcnt[IS_IOV_LDS_SLOTS];
    const int f = blockIdx.x / a.row_groups, rg = blockIdx.x % a.row_groups;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = blockIdx.y * 64 + lane;
    const int y0 = (rg * IS_IOV_WAVES + wave) * IS_IOV_RCH;
    const int y1 = min(y0 + IS_IOV_RCH, a.rows);
    for (int i = threadIdx.x; i < IS_IOV_LDS_SLOTS; i += blockDim.x) {
        lkeys[i] = IOV_EMPTY;
        lcnt[i] = 0;
    }
    __syncthreads();

    u64 run_key = 0;
    unsigned run = 0;
    if (c < a.xlanes && y0 < y1) {
        int16_t* m = &strip[wave][0][lane];
        for (int r = 0; r < IS_IOV_RCH; r++) m[r * 64] = -1;
        const bool stixel = c < a.realcols;
        const size_t colbase = ((size_t)f * a.realcols + (stixel ? c : 0)) * a.max_sections;
        const is_section* col = a.sections + colbase;
        if (stixel)
            for (int i = 0; i < a.max_sections; i++) {
                const int4 h = *(const int4*)&col[i]; /* type, vB, vT, disparity */
                if (h.x == -1) break;
                const long long top = (long long)a.rows - 1 - h.z, bot = (long long)a.rows - 1 - h.y;
                const long long lo = max(top, (long long)y0), hi = min(bot, (long long)y1 - 1);
                if (lo > hi) continue;
                for (int y = (int)lo; y <= (int)hi; y++) m[(y - y0) * 64] = (int16_t)i;
            }
        const int x0 = c * a.w;
        const int npx = stixel ? a.w : a.cols - a.realcols * a.w;
        int cur = -2;
        int32_t iv = 0;
        for (int y = y0; y < y1; y++) {
            const int s = m[(y - y0) * 64];
            if (s != cur) {
                cur = s;
                iv = 0;
                if (s >= 0 && a.section_instance) {
                    const int l = a.section_instance[colbase + s];
                    if (l >= 0 && l < 1000)
                        iv = (int32_t)((uint32_t)col[s].semantic_class * 1000u + (uint32_t)l);
                }
            }
            const size_t pix = ((size_t)f * a.rows + y) * a.cols + x0;
            if (VEC && stixel) {
                const int4 g0 = ((const int4*)(a.gt + pix))[0];
                const int4 g1 = ((const int4*)(a.gt + pix))[1];
                IOV_TALLY(iov_key(iv, g0.x));
                IOV_TALLY(iov_key(iv, g0.y));
                IOV_TALLY(iov_key(iv, g0.z));
                IOV_TALLY(iov_key(iv, g0.w));
                IOV_TALLY(iov_key(iv, g1.x));
                IOV_TALLY(iov_key(iv, g1.y));
                IOV_TALLY(iov_key(iv, g1.z));
                IOV_TALLY(iov_key(iv, g1.w));
            } else {
                for (int k = 0; k < npx; k++) IOV_TALLY(iov_key(iv, a.gt[pix + k]));
            }
        }
    }
    if (run) iov_flush(a, f, lkeys, lcnt, run_key, run);
    __syncthreads();
    for (int i = threadIdx.x; i < IS_IOV_LDS_SLOTS; i += blockDim.x)
        if (lkeys[i] != IOV_EMPTY) iov_global_insert(a, f, lkeys[i], lcnt[i]);
}

/* The non-empty slots of each frame's hash into sortk [n][P] (which holds all-ones on entry). */
__global__ __launch_bounds__(256) void k_iov_gather(const u64* __restrict__ gkeys, int slots_log2, int* fc,
                                                    u64* __restrict__ sortk, int P) {
    const int f = blockIdx.y;
    const unsigned s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= (1u << slots_log2)) return;
    const u64 k = gkeys[((size_t)f << slots_log2) + s];
    if (k == IOV_EMPTY) return;
    const int i = atomicAdd(&fc[(size_t)f * IOV_NCNT + IOV_FILL], 1);
    if (i < P) sortk[(size_t)f * P + i] = k;
}

/* Bitonic sort of [n][P] keys, ascending.  FULL: every stage up to the block (B = blockDim-sized LDS block of
 * `block` keys); else the steps j < block of stage `k`. */
template <bool FULL>
__global__ __launch_bounds__(IS_IOV_SORT_THREADS) void k_iov_sort_local(u64* keys, int P, int block, int k) {
    __shared__ u64 s[IS_IOV_SORT_LDS];
    const int f = blockIdx.y;
    const int base = blockIdx.x * block;
    u64* g = keys + (size_t)f * P + base;
    for (int t = threadIdx.x; t < block; t += blockDim.x) s[t] = g[t];
    __syncthreads();
    for (int size = FULL ? 2 : k; size <= (FULL ? block : k); size <<= 1)
        for (int stride = (FULL ? size : block) >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < block; t += blockDim.x) {
                const int u = t ^ stride;
                if (u > t) {
                    const u64 x = s[t], y = s[u];
                    const bool up = ((base + t) & size) == 0;
                    if ((x > y) == up) {
                        s[t] = y;
                        s[u] = x;
                    }
                }
            }
            __syncthreads();
        }
    for (int t = threadIdx.x; t < block; t += blockDim.x) g[t] = s[t];
}

__global__ __launch_bounds__(256) void k_iov_sort_global(u64* keys, int P, int k, int j) {
    const int f = blockIdx.y;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= P) return;
    const int u = t ^ j;
    if (u <= t) return;
    u64* g = keys + (size_t)f * P;
    const u64 x = g[t], y = g[u];
    const bool up = (t & k) == 0;
    if ((x > y) == up) {
        g[t] = y;
        g[u] = x;
    }
}

/* Records, n_records and overflow of every frame; the count of each sorted key looked up in its hash. */
__global__ __launch_bounds__(256) void k_iov_emit(const u64* __restrict__ gkeys, const unsigned* __restrict__ gcnt,
                                                  int slots_log2, const int* __restrict__ fc,
                                                  const u64* __restrict__ sortk, int P, int capacity,
                                                  is_overlap_record* records, int32_t* n_records,
                                                  int32_t* overflow) {
    const int f = blockIdx.y;
    const int* c = fc + (size_t)f * IOV_NCNT;
    const int distinct = c[IOV_DISTINCT], fill = c[IOV_FILL];
    const unsigned sentinel = (unsigned)c[IOV_SENTINEL];
    const long long total = (long long)distinct + (sentinel ? 1 : 0);
    const bool over = c[IOV_FLAG] != 0 || fill != distinct || total > capacity;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) {
        n_records[f] = over ? 0 : (int32_t)total;
        overflow[f] = over ? 1 : 0;
    }
    if (over || t >= total) return;
    is_overlap_record r;
    if (t == distinct) { /* the all-ones key: pred = gt = INT32_MAX */
        r.pred = 0x7fffffff;
        r.gt = 0x7fffffff;
        r.count = sentinel;
    } else {
        const u64 k = sortk[(size_t)f * P + t];
        const unsigned slots = 1u << slots_log2;
        const u64* keys = gkeys + ((size_t)f << slots_log2);
        unsigned s = iov_hash(k, slots_log2);
        for (unsigned i = 0; i < slots && keys[s] != k; i++) s = (s + 1) & (slots - 1);
        r.pred = (int32_t)((uint32_t)(k >> 32) ^ 0x80000000u);
        r.gt = (int32_t)((uint32_t)k ^ 0x80000000u);
        r.count = gcnt[((size_t)f << slots_log2) + s];
    }
    records[(size_t)f * capacity + t] = r;
}

/* records [n][capacity] -> packed back to back in frame order (n_records[f] of frame f). */
__global__ __launch_bounds__(256) void k_iov_pack(const is_overlap_record* __restrict__ records,
                                                  const int32_t* __restrict__ n_records, int capacity,
                                                  is_overlap_record* __restrict__ packed) {
    const int f = blockIdx.y;
    __shared__ long long off;
    if (threadIdx.x == 0) {
        long long o = 0;
        for (int i = 0; i < f; i++) o += n_records[i];
        off = o;
    }
    __syncthreads();
    const int m = n_records[f];
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < m; t += gridDim.x * blockDim.x)
        packed[off + t] = records[(size_t)f * capacity + t];
}

extern "C" {

/* The arguments are checked by is_instance_overlap. */
hipError_t isk_launch_instance_overlap(const is_instance_overlap_args* r, hipStream_t stream) {
    const int n = r->n_images;
    int P = 1;
    while (P < r->capacity) P <<= 1;
    int log2 = 1;
    while ((1 << log2) < 2 * P) log2++;
    const size_t slots = (size_t)1 << log2;
    /* scratch: [n][slots] keys | [n][P] sort keys (all-ones) | [n][slots] counts | [n][IOV_NCNT] (zero) */
    const size_t ones = (size_t)n * (slots + P) * sizeof(u64);
    const size_t zeros = (size_t)n * slots * sizeof(unsigned) + (size_t)n * IOV_NCNT * sizeof(int);
    void* scratch = nullptr;
    hipError_t e = hipMallocAsync(&scratch, ones + zeros, stream);
    if (e != hipSuccess) return e;
    IovArgs a = {};
    a.sections = r->d_sections;
    a.section_instance = r->d_section_instance;
    a.gt = r->d_gt_instance;
    a.gkeys = (u64*)scratch;
    u64* sortk = a.gkeys + (size_t)n * slots;
    a.gcnt = (unsigned*)((char*)scratch + ones);
    a.fc = (int*)(a.gcnt + (size_t)n * slots);
    a.realcols = r->realcols;
    a.max_sections = r->max_sections;
    a.rows = r->rows;
    a.cols = r->cols;
    a.w = r->cols / r->realcols;
    a.xlanes = r->realcols + (r->cols > r->realcols * a.w ? 1 : 0);
    a.row_groups = (r->rows + IS_IOV_RCH * IS_IOV_WAVES - 1) / (IS_IOV_RCH * IS_IOV_WAVES);
    a.capacity = r->capacity;
    a.slots_log2 = log2;
    e = hipMemsetAsync(scratch, 0xff, ones, stream);
    if (e == hipSuccess) e = hipMemsetAsync((char*)scratch + ones, 0, zeros, stream);
    if (e == hipSuccess) {
        const bool vec = a.w == 8 && a.cols % 8 == 0 && ((uintptr_t)a.gt & 15) == 0;
        const dim3 grid((unsigned)(n * a.row_groups), (unsigned)((a.xlanes + 63) / 64));
        if (vec)
            hipLaunchKernelGGL(k_iov<true>, grid, dim3(64 * IS_IOV_WAVES), 0, stream, a);
        else
            hipLaunchKernelGGL(k_iov<false>, grid, dim3(64 * IS_IOV_WAVES), 0, stream, a);
        hipLaunchKernelGGL(k_iov_gather, dim3((unsigned)((slots + 255) / 256), n), dim3(256), 0, stream, a.gkeys,
                           log2, a.fc, sortk, P);
        const int B = P < IS_IOV_SORT_LDS ? P : IS_IOV_SORT_LDS;
        const int threads = B < IS_IOV_SORT_THREADS ? (B < 64 ? 64 : B) : IS_IOV_SORT_THREADS;
        hipLaunchKernelGGL(k_iov_sort_local<true>, dim3(P / B, n), dim3(threads), 0, stream, sortk, P, B, 0);
        for (int k = 2 * B; k <= P; k <<= 1) {
            for (int j = k >> 1; j >= B; j >>= 1)
                hipLaunchKernelGGL(k_iov_sort_global, dim3((P + 255) / 256, n), dim3(256), 0, stream, sortk, P, k, j);
            hipLaunchKernelGGL(k_iov_sort_local<false>, dim3(P / B, n), dim3(threads), 0, stream, sortk, P, B, k);
        }
        hipLaunchKernelGGL(k_iov_emit, dim3((P + 256) / 256, n), dim3(256), 0, stream, a.gkeys, a.gcnt, log2, a.fc,
                           sortk, P, r->capacity, r->d_records, r->d_n_records, r->d_overflow);
        e = hipGetLastError();
    }
    const hipError_t e2 = hipFreeAsync(scratch, stream);
    return e == hipSuccess ? e2 : e;
}

hipError_t isk_launch_pack_overlap(const is_overlap_record* records, const int32_t* n_records, int n_images,
                                   int capacity, is_overlap_record* packed, hipStream_t stream) {
    const int blocks = (capacity + 255) / 256 < 64 ? (capacity + 255) / 256 : 64;
    hipLaunchKernelGGL(k_iov_pack, dim3(blocks, n_images), dim3(256), 0, stream, records, n_records, capacity,
                       packed);
    return hipGetLastError();
}

} /* extern "C" */
