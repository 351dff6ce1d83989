/*
 * is_k_instance_disparity.hip -- f10: the instance id of every stixel by DBSCAN over (x, y, instance disparity), the
 * third way the reference's evaluation tooling labels stixels (--use-disparity from_gt of
 * tools/visualization/clustering_visualization.py): compute_instance_disparity :1024-1049 over the masks of
 * cityscapes_instance_loader.py load_instance_mask :32-71, add_instance_disparity :996-1022,
 * get_disparity_instance_centers :794-819 and assign_instances :894-960.  The numpy restatement is
 * tests/instance_disparity_reference.py.  Six launches behind one memset, all on the caller's stream:
 *
 *   k_idisp_pixels<., false>  marks the keys of a frame (class index * 1000 + instance number, 8000 of them) in a
 *                             presence bitmap; eight pixels per lane, one atomicOr per run of equal keys;
 *   k_idisp_rank              one workgroup per frame ranks the set bits to slots (key -> slot, slot -> key), reports
 *                             the frame's TRUE key count and raises the batch's overflow word where it exceeds the
 *                             caller's capacity: every later launch then returns at once, nothing is truncated;
 *   k_idisp_pixels<., true>   the same walk again, adding the non-zero disparities into [slot][256] uint32; runs of
 *                             equal (key, disparity) are merged in registers before one atomicAdd.  Integer atomics
 *                             only, so the histograms do not depend on the order of arrival;
 *   k_idisp_key_median        one wave per slot: four bins per lane, a wave scan, the two middle ranks -> their sum,
 *                             the median in HALF units (np.median averages the middle pair), into key -> median;
 *   k_idisp_stixel            the walk of is_stixel_walk.h, one wave per (frame, stixel column): every pixel's value
 *                             is median[key(pixel)], collected in a 512-bin LDS histogram of half units per wave
 *                             (the values < 1, bins 0 and 1, are dropped, :1012-1013), read back interleaved (lane l:
 *                             l, l + 64, ...: conflict-free) and scanned chunk by chunk; the two middle ranks' sum *
 *                             0.25 is the stixel's median, an integer number of quarter units, exact in fp32;
 *   k_idisp_cluster           the clustering of is_dbscan.h over three coordinates: the candidates whose stixel
 *                             median is 0 take no part.  It derives the core-candidate flag as k_recore does and
 *                             writes d_labels, d_core_candidates and d_packed as is_recluster leaves them.
 *
 * The instance-disparity image of the reference is never built: a pixel's value is median[key(pixel)].
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "instance_stixels_core.h"
#include "is_dbscan.h"
#include "is_launch.h"
#include "is_stixel_walk.h"

#define IDK_KEYS IS_INSTANCE_DISPARITY_KEYS
#define IDK_WORDS 256        /* bitmap words per frame: 250 used, one per lane of k_idisp_rank */
#define IDK_BINS 256         /* disparity bins of a slot */
#define IDK_WAVES 4          /* waves per workgroup of k_idisp_key_median and k_idisp_stixel */
#define IDK_HALF_BINS 512    /* per wave: half units 0 .. 510 */
#define IDK_THREADS 256      /* of k_idisp_pixels */
#define IDK_TABLE_IMAGES 32  /* frames per k_idisp_cluster launch: their arrays travel as a kernel argument */

static_assert(IDK_KEYS == 8 * 1000 && IDK_KEYS <= 32 * IDK_WORDS && IDK_KEYS <= 65535, "keys: 8 classes x 1000");

/* The parts of the caller's scratch (idisp_layout); key_count, key_median and stixel are the caller's own arrays
 * where it asked for those outputs. */
struct IdispScratch {
    int* overflow;          /* [4]: word 0 != 0: a frame has more keys than slots, nothing is written */
    unsigned* bitmap;       /* [n][IDK_WORDS] */
    unsigned* hist;         /* [n][capacity][IDK_BINS] */
    uint16_t* slot_of_key;  /* [n][IDK_KEYS], valid for the keys present */
    uint16_t* key_of_slot;  /* [n][capacity] */
    uint16_t* key_median;   /* [n][IDK_KEYS] half units */
    int32_t* key_count;     /* [n] */
    float* stixel;          /* [n][n_slots] */
    float* z;               /* [n][n_slots]: the candidates' medians, class after class */
    int32_t* rank;          /* [n][2][n_slots]: rank | out of the clustering, class after class */
};

struct IdispLayout {
    size_t overflow, bitmap, hist, zero_end, slot_of_key, key_of_slot, key_median, key_count, stixel, z, rank, total;
};

static IdispLayout idisp_layout(size_t n, size_t n_slots, size_t capacity) {
    IdispLayout l;
    size_t o = 0;
    auto take = [&o](size_t bytes) {
        const size_t at = o;
        o += (bytes + 15) & ~(size_t)15;
        return at;
    };
    l.overflow = take(4 * sizeof(int));
    l.bitmap = take(n * IDK_WORDS * sizeof(unsigned));
    l.hist = take(n * capacity * IDK_BINS * sizeof(unsigned));
    l.zero_end = o; /* [0, zero_end) is cleared in front of every call */
    l.slot_of_key = take(n * IDK_KEYS * sizeof(uint16_t));
    l.key_of_slot = take(n * capacity * sizeof(uint16_t));
    l.key_median = take(n * IDK_KEYS * sizeof(uint16_t));
    l.key_count = take(n * sizeof(int32_t));
    l.stixel = take(n * n_slots * sizeof(float));
    l.z = take(n * n_slots * sizeof(float));
    l.rank = take(n * 2 * n_slots * sizeof(int32_t));
    l.total = o;
    return l;
}

/* The key of a ground-truth pixel: id > 1000 and id / 1000 one of the labelIds 24..28, 31..33 of classes 11..18
 * (cityscapes_instance_loader.py:45); the instance number 0 (labelId * 1000) is a key like any other.  -1: none. */
__device__ __forceinline__ int idk_key(int v) {
    if (v <= 1000) return -1;
    const unsigned L = (unsigned)v / 1000u;
    int ci;
    if (L >= 24u && L <= 28u)
        ci = (int)L - 24;
    else if (L >= 31u && L <= 33u)
        ci = (int)L - 26;
    else
        return -1;
    return ci * 1000 + (int)((unsigned)v - L * 1000u);
}

struct IdispPixArgs {
    const int32_t* gt;
    const uint8_t* disp;
    int rows, cols, chunks, capacity; /* chunks: pieces of eight pixels per row */
    size_t frame_px;
    IdispScratch s;
};

/* One lane per eight consecutive pixels of a row, grid = (pieces of a frame / 256, n_images).
 * VEC: cols % 8 == 0, the ground truth 16-byte and the disparity 8-byte aligned: two 16-byte loads and one of 8 bytes.
 * HIST = false marks the keys, HIST = true adds the disparities of the keys' slots. */
template <bool VEC, bool HIST>
__global__ __launch_bounds__(IDK_THREADS) void k_idisp_pixels(const IdispPixArgs a) {
    if (HIST && a.s.overflow[0]) return;
    const int f = blockIdx.y;
    const long long t = (long long)blockIdx.x * IDK_THREADS + threadIdx.x;
    if (t >= (long long)a.rows * a.chunks) return;
    const int y = (int)(t / a.chunks), x0 = (int)(t % a.chunks) * 8;
    const size_t off = (size_t)f * a.frame_px + (size_t)y * a.cols + x0;
    int v[8];
    unsigned d[8];
    if (VEC) {
        const int4 p = *(const int4*)(a.gt + off), q = *(const int4*)(a.gt + off + 4);
        v[0] = p.x; v[1] = p.y; v[2] = p.z; v[3] = p.w;
        v[4] = q.x; v[5] = q.y; v[6] = q.z; v[7] = q.w;
        if (HIST) {
            const uint2 b = *(const uint2*)(a.disp + off);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                d[k] = (b.x >> (8 * k)) & 255u;
                d[4 + k] = (b.y >> (8 * k)) & 255u;
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const bool in = x0 + k < a.cols;
            v[k] = in ? a.gt[off + k] : 0;
            if (HIST) d[k] = in ? a.disp[off + k] : 0u;
        }
    }
    if (!HIST) {
        unsigned* const words = a.s.bitmap + (size_t)f * IDK_WORDS;
        int prev = -1;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int key = idk_key(v[k]);
            if (key >= 0 && key != prev) atomicOr(&words[key >> 5], 1u << (key & 31));
            prev = key;
        }
        return;
    }
    const uint16_t* const slots = a.s.slot_of_key + (size_t)f * IDK_KEYS;
    unsigned* const hist = a.s.hist + (size_t)f * a.capacity * IDK_BINS;
    int run_key = -1;
    unsigned run_d = 0, run = 0;
#pragma unroll
    for (int k = 0; k <= 8; k++) {
        int key = -1;
        unsigned dk = 0;
        if (k < 8) {
            dk = d[k];
            key = dk ? idk_key(v[k]) : -1; /* a zero disparity is not part of any median */
        }
        if (key >= 0 && key == run_key && dk == run_d) {
            run++;
            continue;
        }
        if (run) {
            const int slot = slots[run_key];
            if (slot < a.capacity) atomicAdd(&hist[(size_t)slot * IDK_BINS + run_d], run);
        }
        run_key = key;
        run_d = dk;
        run = key >= 0 ? 1u : 0u;
    }
}

/* One workgroup per frame, one bitmap word per lane: the set bits in ascending key order are the slots. */
__global__ __launch_bounds__(IDK_WORDS) void k_idisp_rank(const IdispScratch s, int capacity) {
    __shared__ int s_cnt[IDK_WORDS];
    const int f = blockIdx.x, t = threadIdx.x;
    const unsigned w = s.bitmap[(size_t)f * IDK_WORDS + t];
    const int mine = __popc(w);
    s_cnt[t] = mine;
    __syncthreads();
    for (int o = 1; o < IDK_WORDS; o <<= 1) {
        const int add = t >= o ? s_cnt[t - o] : 0;
        __syncthreads();
        s_cnt[t] += add;
        __syncthreads();
    }
    int slot = s_cnt[t] - mine;
    const int total = s_cnt[IDK_WORDS - 1];
    if (t == 0) {
        s.key_count[f] = total;
        if (total > capacity) s.overflow[0] = 1;
    }
    uint16_t* const slot_of_key = s.slot_of_key + (size_t)f * IDK_KEYS;
    uint16_t* const key_of_slot = s.key_of_slot + (size_t)f * capacity;
    uint16_t* const median = s.key_median + (size_t)f * IDK_KEYS;
    for (int b = 0; b < 32; b++) {
        const int key = t * 32 + b;
        if (key >= IDK_KEYS) break;
        median[key] = 0; /* a key that is absent, or has no non-zero disparity */
        if (!((w >> b) & 1u)) continue;
        if (slot < capacity) {
            slot_of_key[key] = (uint16_t)slot;
            key_of_slot[slot] = (uint16_t)key;
        }
        slot++;
    }
}

/* inclusive prefix sum over the 64 lanes */
__device__ __forceinline__ unsigned idk_wave_scan(unsigned x, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(x, o, 64);
        if (lane >= o) x += up;
    }
    return x;
}

/* One wave per slot: the median of the slot's histogram in half units. */
__global__ __launch_bounds__(64 * IDK_WAVES) void k_idisp_key_median(const IdispScratch s, int capacity) {
    if (s.overflow[0]) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, f = blockIdx.y;
    const int slot = blockIdx.x * IDK_WAVES + wave;
    if (slot >= min(s.key_count[f], capacity)) return; /* (whole waves; the kernel has no workgroup barrier) */
    const uint4 c = ((const uint4*)(s.hist + ((size_t)f * capacity + slot) * IDK_BINS))[lane];
    const unsigned c0 = lane ? c.x : 0u, c1 = c.y, c2 = c.z, c3 = c.w; /* (bin 0 is never added to) */
    const unsigned sum = c0 + c1 + c2 + c3;
    const unsigned incl = idk_wave_scan(sum, lane);
    const unsigned N = __shfl(incl, 63, 64);
    unsigned half = 0;
    if (N) {
        const unsigned r[2] = {(N - 1) / 2, N / 2}; /* the middle pair; the same rank twice for an odd count */
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const unsigned excl = incl - sum;
            const bool hit = excl <= r[k] && r[k] < incl;
            const unsigned rr = r[k] - excl;
            const int bin = 4 * lane + (rr < c0 ? 0 : rr < c0 + c1 ? 1 : rr < c0 + c1 + c2 ? 2 : 3);
            const uint64_t at = __ballot(hit);
            half += (unsigned)__shfl(bin, __builtin_ctzll(at), 64);
        }
    }
    if (lane == 0) s.key_median[(size_t)f * IDK_KEYS + s.key_of_slot[(size_t)f * capacity + slot]] = (uint16_t)half;
}

struct IdispStixelArgs {
    const is_section* sections;
    const int32_t* gt;
    int realcols, S, rows, cols, w, col_groups;
    IdispScratch s;
};

/* VEC: as isw_tally */
template <bool VEC>
__global__ __launch_bounds__(64 * IDK_WAVES) void k_idisp_stixel(const IdispStixelArgs a) {
    __shared__ unsigned s_bins[IDK_WAVES][IDK_HALF_BINS];
    if (a.s.overflow[0]) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int f = blockIdx.x / a.col_groups;
    const int c = (blockIdx.x % a.col_groups) * IDK_WAVES + wave;
    if (c >= a.realcols) return; /* (whole waves; the kernel has no workgroup barrier) */
    unsigned* const bins = s_bins[wave];
    for (int i = lane; i < IDK_HALF_BINS; i += 64) bins[i] = 0;
    isw_wave_sync();

    const size_t column = ((size_t)f * a.realcols + c) * a.S;
    const is_section* const col = a.sections + column;
    const int32_t* const img = a.gt + (size_t)f * a.rows * a.cols + (size_t)c * a.w;
    const uint16_t* const median = a.s.key_median + (size_t)f * IDK_KEYS;
    bool open = true; /* no terminator so far */
    for (int base = 0; base < a.S; base += 64) {
        const int i = base + lane;
        float result = 0.0f;
        int vB, vT, cls;
        uint64_t todo = isw_round(col, i, a.S, open, vB, vT, cls);
        while (todo) {
            const int src = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int sB = __shfl(vB, src, 64), sT = __shfl(vT, src, 64);
            const auto half_units = [median](int v) { /* values < 1 are dropped (:1012-1013): MIN_BIN = 2 */
                const int g = idk_key(v);
                return g >= 0 ? (unsigned)median[g] : 0u;
            };
            if (!isw_tally<VEC, 2>(img, a.rows, a.cols, a.w, sB, sT, lane, bins, half_units)) continue; /* empty: 0 */
            /* the bins in chunks of 64, lane l the bin 64 j + l of chunk j; incl: the prefix in bin order */
            unsigned n[IDK_HALF_BINS / 64], incl[IDK_HALF_BINS / 64], N = 0;
#pragma unroll
            for (int j = 0; j < IDK_HALF_BINS / 64; j++) {
                n[j] = bins[64 * j + lane];
                if (n[j]) bins[64 * j + lane] = 0;
                const unsigned sc = idk_wave_scan(n[j], lane);
                incl[j] = N + sc;
                N += __shfl(sc, 63, 64);
            }
            isw_wave_sync();
            unsigned half = 0;
            if (N) {
                const unsigned r[2] = {(N - 1) / 2, N / 2};
#pragma unroll
                for (int k = 0; k < 2; k++) {
#pragma unroll
                    for (int j = 0; j < IDK_HALF_BINS / 64; j++) {
                        const uint64_t at = __ballot(incl[j] - n[j] <= r[k] && r[k] < incl[j]);
                        if (at) half += 64u * j + (unsigned)__builtin_ctzll(at);
                    }
                }
            }
            if (lane == src) result = (float)half * 0.25f; /* (half units + half units) / 4 */
        }
        if (i < a.S) a.s.stixel[column + i] = result;
    }
}

/* ---- the clustering: dbs_body (is_dbscan.h) over (x, y, stixel median) ---- */
struct IdispTable {
    is_instance_buffers ib[IDK_TABLE_IMAGES];
};

/* One workgroup per (instance class, frame): grid = (8, frames of the launch). */
__global__ __launch_bounds__(DBS_THREADS) void k_idisp_cluster(const IdispTable tbl, int first_image, int n_slots,
                                                               int S, int size_filter, float eps2, int min_pts,
                                                               const is_section* __restrict__ sections,
                                                               const IdispScratch s) {
    __shared__ int s_red[DBS_THREADS];
    __shared__ dbs_f2 s_xy[DBS_LDS_N];
    __shared__ float s_z[DBS_LDS_N];
    __shared__ int32_t s_lab[DBS_LDS_N];
    __shared__ uint8_t s_cand[DBS_LDS_N];
    if (s.overflow[0]) return;
    const int cls = blockIdx.x, img = first_image + (int)blockIdx.y, tid = threadIdx.x;
    const is_instance_buffers ib = tbl.ib[blockIdx.y];
    const int32_t* per_class = ib.d_instances_per_class;
    const int n = dbs_class_count(per_class, cls, n_slots);
    int base = 0, total = 0;
    DBS_CLASS_RANGE(per_class, cls, n_slots, base, total);
    const size_t o = (size_t)cls * n_slots;
    const dbs_f2* xy = reinterpret_cast<const dbs_f2*>(ib.d_centerofmass) + o;
    uint8_t* cand = ib.d_core_candidates + o;
    int32_t* labels = ib.d_labels + o;
    const int32_t* idx = ib.d_indices + o * 2;
    /* the candidates of a frame are sections of it, each of one class: class after class they fit n_slots entries */
    if (base + n <= n_slots) {
        float* z = s.z + (size_t)img * n_slots + base;
        int32_t* rank = s.rank + (size_t)img * 2 * n_slots + base;
        const is_section* frame = sections + (size_t)img * n_slots;
        const float* stixel = s.stixel + (size_t)img * n_slots;
        for (int i = tid; i < n; i += DBS_THREADS) {
            const int c = idx[2 * i], si = idx[2 * i + 1];
            float zz = 0.0f;
            if (IS_FRAME_SLOT(c, si, S, n_slots)) {
                const is_section* sec = frame + (size_t)c * S + si;
                cand[i] = is_core_candidate(sec->vB, sec->vT, size_filter);
                zz = stixel[(size_t)c * S + si];
            }
            z[i] = zz;
        }
        __syncthreads();
        if (n == 0) {
        } else if (n <= DBS_LDS_N) {
            for (int i = tid; i < n; i += DBS_THREADS) { s_xy[i] = xy[i]; s_z[i] = z[i]; s_cand[i] = cand[i]; }
            __syncthreads();
            dbs_body(n, eps2, min_pts,
                     dbs_points3<const lds_float2*, const lds_float*>{(const lds_float2*)s_xy, (const lds_float*)s_z},
                     (const lds_u8*)s_cand, (lds_i32*)s_lab, labels, rank, rank + n_slots, s_red);
        } else {
            dbs_body(n, eps2, min_pts, dbs_points3<const dbs_f2*, const float*>{xy, z}, (const uint8_t*)cand, labels,
                     labels, rank, rank + n_slots, s_red);
        }
    } else {
        for (int i = tid; i < n; i += DBS_THREADS) labels[i] = -1;
    }
    int32_t* packed = ib.d_packed;
    if (packed) {
        __syncthreads();
        DBS_EMIT_PACKED(packed, cls, n, base, total, idx, labels);
    }
}

extern "C" {

size_t isk_instance_disparity_scratch_bytes(int n_images, int realcols, int max_sections, int capacity) {
    return idisp_layout((size_t)n_images, (size_t)realcols * max_sections, (size_t)capacity).total;
}

/* The arguments are checked by is_cluster_instance_disparity. */
hipError_t isk_launch_instance_disparity(const is_instance_disparity_args* r, hipStream_t stream) {
    const int n = r->n_images, n_slots = r->realcols * r->max_sections, cap = r->capacity;
    const IdispLayout l = idisp_layout((size_t)n, (size_t)n_slots, (size_t)cap);
    char* const base = (char*)r->d_scratch;
    IdispScratch s;
    s.overflow = (int*)(base + l.overflow);
    s.bitmap = (unsigned*)(base + l.bitmap);
    s.hist = (unsigned*)(base + l.hist);
    s.slot_of_key = (uint16_t*)(base + l.slot_of_key);
    s.key_of_slot = (uint16_t*)(base + l.key_of_slot);
    s.key_median = r->d_key_median ? r->d_key_median : (uint16_t*)(base + l.key_median);
    s.key_count = r->d_key_count ? r->d_key_count : (int32_t*)(base + l.key_count);
    s.stixel = r->d_stixel_median ? r->d_stixel_median : (float*)(base + l.stixel);
    s.z = (float*)(base + l.z);
    s.rank = (int32_t*)(base + l.rank);
    hipError_t e = hipMemsetAsync(base, 0, l.zero_end, stream);
    if (e != hipSuccess) return e;

    IdispPixArgs p = {};
    p.gt = r->d_gt_instance;
    p.disp = r->d_disparity_u8;
    p.rows = r->rows;
    p.cols = r->cols;
    p.chunks = (r->cols + 7) / 8;
    p.capacity = cap;
    p.frame_px = (size_t)r->rows * r->cols;
    p.s = s;
    const bool vec = r->cols % 8 == 0 && ((uintptr_t)p.gt & 15) == 0 && ((uintptr_t)p.disp & 7) == 0;
    const dim3 pix_grid((unsigned)(((long long)p.rows * p.chunks + IDK_THREADS - 1) / IDK_THREADS), (unsigned)n);
    if (vec)
        hipLaunchKernelGGL((k_idisp_pixels<true, false>), pix_grid, dim3(IDK_THREADS), 0, stream, p);
    else
        hipLaunchKernelGGL((k_idisp_pixels<false, false>), pix_grid, dim3(IDK_THREADS), 0, stream, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_idisp_rank, dim3((unsigned)n), dim3(IDK_WORDS), 0, stream, s, cap);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (vec)
        hipLaunchKernelGGL((k_idisp_pixels<true, true>), pix_grid, dim3(IDK_THREADS), 0, stream, p);
    else
        hipLaunchKernelGGL((k_idisp_pixels<false, true>), pix_grid, dim3(IDK_THREADS), 0, stream, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_idisp_key_median, dim3((unsigned)((cap + IDK_WAVES - 1) / IDK_WAVES), (unsigned)n),
                       dim3(64 * IDK_WAVES), 0, stream, s, cap);
    if ((e = hipGetLastError()) != hipSuccess) return e;

    IdispStixelArgs a = {};
    a.sections = r->d_sections;
    a.gt = r->d_gt_instance;
    a.realcols = r->realcols;
    a.S = r->max_sections;
    a.rows = r->rows;
    a.cols = r->cols;
    a.w = r->cols / r->realcols;
    a.col_groups = (r->realcols + IDK_WAVES - 1) / IDK_WAVES;
    a.s = s;
    const bool svec = a.w == 8 && a.cols % 8 == 0 && ((uintptr_t)a.gt & 15) == 0;
    const dim3 st_grid((unsigned)(n * a.col_groups));
    if (svec)
        hipLaunchKernelGGL(k_idisp_stixel<true>, st_grid, dim3(64 * IDK_WAVES), 0, stream, a);
    else
        hipLaunchKernelGGL(k_idisp_stixel<false>, st_grid, dim3(64 * IDK_WAVES), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;

    for (int first = 0; first < n; first += IDK_TABLE_IMAGES) {
        const int m = n - first < IDK_TABLE_IMAGES ? n - first : IDK_TABLE_IMAGES;
        IdispTable tbl = {};
        for (int i = 0; i < m; i++) tbl.ib[i] = r->instances[first + i];
        hipLaunchKernelGGL(k_idisp_cluster, dim3(IS_INSTANCE_CLASSES, (unsigned)m), dim3(DBS_THREADS), 0, stream, tbl,
                           first, n_slots, r->max_sections, r->size_filter, r->eps * r->eps, r->min_pts,
                           r->d_sections, s);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

} /* extern "C" */
