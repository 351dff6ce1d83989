/*
 * is_k_gt_targets.hip -- f11: the ground-truth offset targets of the reference's CNN for a batch, and the same values
 * as the two offset channels of a DP input (is_mode_downsample, is_gt_instance_targets of instance_stixels_core.h).
 * It replaces the Python loops of the reference's training data set (tools/CNN_training/datasets/transforms.py
 * modefilter_np :59-70, datasets/cityscapes.py _instance_offsets_disparity :114-144 and _instance_offsets :146-167)
 * and the "gt offsets" row of its instance evaluation (tools/CNN_training/inference.py:388-396 behind
 * tools/run_cityscapes.py --usegtoffsets).  The numpy restatement is tests/gt_targets_reference.py.  On the caller's
 * stream, behind one memset:
 *
 *   k_mode_downsample<T, .>   one lane per cell of 8x8 pixels, 64 adjacent cells of a cell row per wave.  The 64 values
 *                             of a cell stay in registers; a cell whose values are all equal is done at once, any
 *                             other one is sorted by a bitonic network over those registers and the longest run of
 *                             the sorted values wins, the first (smallest) one among equals;
 *   k_gtt_moments             one lane per cell: runs of equal ids along a wave's cells are tallied in registers
 *                             (count, sum of rows, sum of columns in closed form), then one update per run of the
 *                             frame's open-addressing table: compare-and-swap for the slot, integer atomic adds for
 *                             the three sums, so the sums do not depend on the order of arrival.  The lane that
 *                             claims a slot numbers the key: the frame's key count;
 *   k_gtt_hist                (disparity only) the cells' q = v / 256 into [key number][256] uint32, one add per run
 *                             of equal (id, q);
 *   k_gtt_median              (disparity only) one wave per key: the LOWER median of its histogram (torch.median);
 *   k_gtt_emit                tiles of 64 x 64 cells: in image order the float targets and the ids, then through LDS
 *                             with a lane per row h' = Hs-1-y the two segmentation channels, 256 contiguous bytes per
 *                             store, the padding rows included.
 *
 * A frame with more keys than histograms raises the batch's overflow word in k_gtt_moments; k_gtt_hist, k_gtt_median
 * and k_gtt_emit then return at once (after k_gtt_emit has reported the key counts).
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "instance_stixels_core.h"
#include "is_gt_keys.h"
#include "is_launch.h"

#define GTT_THREADS 256
#define GTT_WAVES (GTT_THREADS / 64)
#define GTT_TILE 64

struct GttScratch {
    int* overflow;     /* [4]: word 0 != 0: a frame has more keys than histograms, no output is written */
    int32_t* count;    /* [n] keys per frame */
    GttEntry* table;   /* [n][slots] */
    unsigned* hist;    /* [n][capacity][GTT_BINS] */
    int32_t* median;   /* [n][capacity] */
    int32_t* ids;      /* [n][Hs][Ws] */
    uint16_t* disp;    /* [n][Hs][Ws] */
};

struct GttLayout {
    size_t overflow, count, table, hist, zero_end, median, ids, disp, total;
};

static GttLayout gtt_layout(size_t n, size_t cells, bool disparity, size_t capacity) {
    GttLayout l;
    size_t o = 0;
    auto take = [&o](size_t bytes) {
        const size_t at = o;
        o += (bytes + 15) & ~(size_t)15;
        return at;
    };
    l.overflow = take(4 * sizeof(int));
    l.count = take(n * sizeof(int32_t));
    l.table = take(n * ((size_t)1 << gtt_log_slots(cells)) * sizeof(GttEntry));
    l.hist = take(disparity ? n * capacity * GTT_BINS * sizeof(unsigned) : 0);
    l.zero_end = o; /* [0, zero_end) is cleared in front of every call */
    l.median = take(disparity ? n * capacity * sizeof(int32_t) : 0);
    l.ids = take(n * cells * sizeof(int32_t));
    l.disp = take(disparity ? n * cells * sizeof(uint16_t) : 0);
    l.total = o;
    return l;
}

/* ---- step 1: the mode of every 8x8 block ---- */

/* v[0..63] ascending: a bitonic network, every index a compile-time constant (the values stay in registers) */
__device__ __forceinline__ void gtt_sort64(int (&v)[64]) {
#pragma unroll
    for (int lk = 1; lk <= 6; lk++) {
#pragma unroll
        for (int lj = lk - 1; lj >= 0; lj--) {
#pragma unroll
            for (int i = 0; i < 64; i++) {
                const int k = 1 << lk, j = 1 << lj, l = i ^ j;
                if (l > i) {
                    const int lo = min(v[i], v[l]), hi = max(v[i], v[l]);
                    const bool up = (i & k) == 0;
                    v[i] = up ? lo : hi;
                    v[l] = up ? hi : lo;
                }
            }
        }
    }
}

/* the most frequent of 64 values, the smallest among equals (np.bincount(..).argmax()) */
__device__ __forceinline__ int gtt_mode64(int (&v)[64]) {
    int differ = 0;
#pragma unroll
    for (int i = 1; i < 64; i++) differ |= v[i] ^ v[0];
    if (!differ) return v[0];
    gtt_sort64(v);
    int best = v[0], best_n = 0, run = 1;
#pragma unroll
    for (int i = 1; i < 64; i++) {
        const bool same = v[i] == v[i - 1];
        if (!same && run > best_n) {
            best_n = run;
            best = v[i - 1];
        }
        run = same ? run + 1 : 1;
    }
    return run > best_n ? v[63] : best;
}

template <class T> struct GttVec;
template <> struct GttVec<int32_t> {
    static __device__ __forceinline__ void load(const int32_t* p, int* v) {
        const int4 a = *(const int4*)p, b = *(const int4*)(p + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
};
template <> struct GttVec<uint16_t> {
    static __device__ __forceinline__ void load(const uint16_t* p, int* v) {
        const uint4 a = *(const uint4*)p;
        const unsigned w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            v[2 * k] = (int)(w[k] & 0xffffu);
            v[2 * k + 1] = (int)(w[k] >> 16);
        }
    }
};
template <> struct GttVec<uint8_t> {
    static __device__ __forceinline__ void load(const uint8_t* p, int* v) {
        const uint2 a = *(const uint2*)p;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            v[k] = (int)((a.x >> (8 * k)) & 255u);
            v[4 + k] = (int)((a.y >> (8 * k)) & 255u);
        }
    }
};

/* One wave per 64 adjacent cells of a cell row: wave w of the grid is (frame, cell row, chunk) = w / (Hs * chunks),
 * ...  VEC: src is 16-byte aligned (cols % 8 == 0 always): one cell's eight values of an image row in one or two
 * vector loads. */
template <class T, bool VEC>
__global__ __launch_bounds__(GTT_THREADS) void k_mode_downsample(const T* __restrict__ src, T* __restrict__ dst,
                                                                 int Hs, int Ws, int chunks, long long waves) {
    const long long w = (long long)blockIdx.x * GTT_WAVES + (threadIdx.x >> 6);
    if (w >= waves) return;
    const int lane = threadIdx.x & 63;
    const int chunk = (int)(w % chunks);
    const long long fy = w / chunks; /* frame * Hs + cell row: the frames are contiguous */
    const int x = chunk * 64 + lane;
    if (x >= Ws) return;
    const size_t cols = (size_t)Ws * 8;
    const T* p = src + (size_t)fy * 8 * cols + (size_t)x * 8;
    int v[64];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        if (VEC) {
            GttVec<T>::load(p + r * cols, v + 8 * r);
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++) v[8 * r + k] = (int)p[r * cols + k];
        }
    }
    dst[(size_t)fy * Ws + x] = (T)gtt_mode64(v);
}

template <class T>
static hipError_t gtt_launch_mode(const T* src, T* dst, int n, int Hs, int Ws, hipStream_t stream) {
    const int chunks = (Ws + 63) / 64;
    const long long waves = (long long)n * Hs * chunks;
    const dim3 grid((unsigned)((waves + GTT_WAVES - 1) / GTT_WAVES));
    if (((uintptr_t)src & 15) == 0)
        hipLaunchKernelGGL((k_mode_downsample<T, true>), grid, dim3(GTT_THREADS), 0, stream, src, dst, Hs, Ws, chunks,
                           waves);
    else
        hipLaunchKernelGGL((k_mode_downsample<T, false>), grid, dim3(GTT_THREADS), 0, stream, src, dst, Hs, Ws, chunks,
                           waves);
    return hipGetLastError();
}

/* ---- steps 2 and 3: keys and their moments ---- */

struct GttArgs {
    GttScratch s;
    int Hs, Ws, chunks, capacity, disparity;
    unsigned log_slots;
    long long waves;
    /* k_gtt_emit */
    float* targets;
    int planes;
    int32_t* ids8;
    int32_t* seg;
    int P2S;
    int32_t* key_count;
};

/* The wave's cell of this lane, as k_mode_downsample maps them.  False: no cell. */
__device__ __forceinline__ bool gtt_cell(const GttArgs& a, long long& w, int& f, int& y, int& x) {
    w = (long long)blockIdx.x * GTT_WAVES + (threadIdx.x >> 6);
    if (w >= a.waves) return false;
    const long long fy = w / a.chunks;
    f = (int)(fy / a.Hs);
    y = (int)(fy % a.Hs);
    x = (int)(w % a.chunks) * 64 + (int)(threadIdx.x & 63);
    return true;
}

__global__ __launch_bounds__(GTT_THREADS) void k_gtt_moments(const GttArgs a) {
    long long w;
    int f, y, x;
    if (!gtt_cell(a, w, f, y, x)) return; /* (whole waves) */
    const int lane = threadIdx.x & 63;
    const size_t cells = (size_t)a.Hs * a.Ws;
    int key = 0;
    if (x < a.Ws) {
        const int id = a.s.ids[(size_t)f * cells + (size_t)y * a.Ws + x];
        if (id > 1000) key = id;
    }
    const int before = __shfl_up(key, 1, 64);
    int next;
    if (!gtt_run_head(key != before, key != 0, lane, next)) return;
    const unsigned long long len = (unsigned long long)(next - lane);
    const unsigned long long x0 = (unsigned long long)(x - lane);
    /* columns x0 + lane .. x0 + next - 1 */
    const unsigned long long sx = len * x0 + (unsigned long long)(lane + next - 1) * len / 2;
    GttEntry* const table = a.s.table + ((size_t)f << a.log_slots);
    int fresh;
    const unsigned at = gtt_enter(table, a.log_slots, key, &a.s.count[f], fresh);
    if (a.disparity && fresh >= a.capacity) a.s.overflow[0] = 1;
    atomicAdd(&table[at].n, (unsigned)len);
    atomicAdd(&table[at].sy, len * (unsigned long long)y);
    atomicAdd(&table[at].sx, sx);
}

/* ---- step 4: the keys' median disparities ---- */
__global__ __launch_bounds__(GTT_THREADS) void k_gtt_hist(const GttArgs a) {
    if (a.s.overflow[0]) return;
    long long w;
    int f, y, x;
    if (!gtt_cell(a, w, f, y, x)) return;
    const int lane = threadIdx.x & 63;
    const size_t cells = (size_t)a.Hs * a.Ws;
    int key = 0, q = 0;
    if (x < a.Ws) {
        const size_t at = (size_t)f * cells + (size_t)y * a.Ws + x;
        const int id = a.s.ids[at];
        q = (int)a.s.disp[at] >> 8;
        if (id > 1000 && q != 0) key = id; /* a zero is not part of any median */
    }
    const int key_before = __shfl_up(key, 1, 64), q_before = __shfl_up(q, 1, 64);
    int next;
    if (!gtt_run_head(key != key_before || q != q_before, key != 0, lane, next)) return;
    const GttEntry* e = gtt_find(a.s.table + ((size_t)f << a.log_slots), a.log_slots, key);
    if (!e || e->number >= a.capacity) return;
    atomicAdd(&a.s.hist[((size_t)f * a.capacity + e->number) * GTT_BINS + q], (unsigned)(next - lane));
}

/* One wave per key number: the lower median of its histogram. */
__global__ __launch_bounds__(GTT_THREADS) void k_gtt_median(const GttArgs a) {
    if (a.s.overflow[0]) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, f = blockIdx.y;
    const int number = blockIdx.x * GTT_WAVES + wave;
    if (number >= min(a.s.count[f], a.capacity)) return; /* (whole waves; the kernel has no workgroup barrier) */
    unsigned N;
    const int median = gtt_lower_median(a.s.hist + ((size_t)f * a.capacity + number) * GTT_BINS, lane, N);
    if (lane == 0) a.s.median[(size_t)f * a.capacity + number] = median;
}

/* ---- steps 3 to 5: the outputs.  grid = (ceil(Ws / 64), ceil(rows of h' / 64), n): tile row j is h' = 64 ty + j,
 * the cell row y = Hs - 1 - h'; with a segmentation h' runs to P2S, the rows from Hs on hold no cell. ---- */
__global__ __launch_bounds__(GTT_THREADS) void k_gtt_emit(const GttArgs a) {
    __shared__ int s_y[GTT_TILE][GTT_TILE + 1], s_x[GTT_TILE][GTT_TILE + 1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, f = blockIdx.z;
    if (a.key_count && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) a.key_count[f] = a.s.count[f];
    if (a.s.overflow[0]) return; /* (the whole grid alike) */
    const size_t cells = (size_t)a.Hs * a.Ws;
    const GttEntry* const table = a.s.table + ((size_t)f << a.log_slots);
    const int x = blockIdx.x * GTT_TILE + lane;
    for (int j = wave; j < GTT_TILE; j += GTT_WAVES) {
        const int h = blockIdx.y * GTT_TILE + j;
        int iy = 0, ix = 0;
        if (h < a.Hs && x < a.Ws) {
            const int y = a.Hs - 1 - h;
            const size_t cell = (size_t)y * a.Ws + x;
            const int id = a.s.ids[(size_t)f * cells + cell];
            float off_y = 0.0f, off_x = 0.0f, med = 0.0f;
            if (id > 1000) {
                const GttEntry* e = gtt_find(table, a.log_slots, id);
                if (e) {
                    const float n = (float)e->n;
                    off_y = (float)e->sy / n - (float)y;
                    off_x = (float)e->sx / n - (float)x;
                    if (a.planes == 3) med = (float)a.s.median[(size_t)f * a.capacity + e->number];
                }
            }
            if (a.targets) {
                float* t = a.targets + (size_t)f * a.planes * cells + cell;
                if (a.planes == 3) {
                    t[0] = med;
                    t += cells;
                }
                t[0] = off_y;
                t[cells] = off_x;
            }
            if (a.ids8) a.ids8[(size_t)f * cells + cell] = id;
            iy = (int)(8.0f * off_y);
            ix = (int)(8.0f * off_x);
        }
        s_y[j][lane] = iy;
        s_x[j][lane] = ix;
    }
    if (!a.seg) return; /* (the whole grid alike) */
    __syncthreads();
    const int h = blockIdx.y * GTT_TILE + lane;
    if (h >= a.P2S) return;
    for (int i = wave; i < GTT_TILE; i += GTT_WAVES) {
        const int col = blockIdx.x * GTT_TILE + i;
        if (col >= a.Ws) break;
        int32_t* o = a.seg + (((size_t)f * a.Ws + col) * IS_GT_TARGETS_CHANNELS + (IS_GT_TARGETS_CHANNELS - 2)) * a.P2S + h;
        o[0] = s_y[lane][i];
        o[a.P2S] = s_x[lane][i];
    }
}

extern "C" {

hipError_t isk_launch_mode_downsample(const void* src, int dtype, int n, int Hs, int Ws, void* dst,
                                      hipStream_t stream) {
    switch (dtype) {
    case IS_DTYPE_INT32: return gtt_launch_mode((const int32_t*)src, (int32_t*)dst, n, Hs, Ws, stream);
    case IS_DTYPE_UINT16: return gtt_launch_mode((const uint16_t*)src, (uint16_t*)dst, n, Hs, Ws, stream);
    default: return gtt_launch_mode((const uint8_t*)src, (uint8_t*)dst, n, Hs, Ws, stream);
    }
}

size_t isk_gt_targets_scratch_bytes(int n_images, int Hs, int Ws, int disparity, int capacity) {
    return gtt_layout((size_t)n_images, (size_t)Hs * Ws, disparity != 0, (size_t)capacity).total;
}

/* The arguments are checked by is_gt_instance_targets; capacity is the effective one. */
hipError_t isk_launch_gt_targets(const is_gt_targets_args* r, int capacity, hipStream_t stream) {
    const int n = r->n_images, Hs = r->rows / 8, Ws = r->cols / 8;
    const bool disparity = r->d_disparity_u16 != nullptr;
    const size_t cells = (size_t)Hs * Ws;
    const GttLayout l = gtt_layout((size_t)n, cells, disparity, (size_t)capacity);
    char* const base = (char*)r->d_scratch;
    GttArgs a = {};
    a.s.overflow = (int*)(base + l.overflow);
    a.s.count = (int32_t*)(base + l.count);
    a.s.table = (GttEntry*)(base + l.table);
    a.s.hist = (unsigned*)(base + l.hist);
    a.s.median = (int32_t*)(base + l.median);
    a.s.ids = (int32_t*)(base + l.ids);
    a.s.disp = (uint16_t*)(base + l.disp);
    a.Hs = Hs;
    a.Ws = Ws;
    a.chunks = (Ws + 63) / 64;
    a.capacity = capacity;
    a.disparity = disparity;
    a.log_slots = gtt_log_slots(cells);
    a.waves = (long long)n * Hs * a.chunks;
    a.targets = r->d_targets;
    a.planes = r->d_targets ? r->target_planes : 2;
    a.ids8 = r->d_ids8;
    a.seg = r->d_segmentation;
    a.P2S = r->rows_power2_segmentation;
    a.key_count = r->d_key_count;
    hipError_t e = hipMemsetAsync(base, 0, l.zero_end, stream);
    if (e != hipSuccess) return e;
    if ((e = gtt_launch_mode(r->d_gt_instance, a.s.ids, n, Hs, Ws, stream)) != hipSuccess) return e;
    const dim3 cell_grid((unsigned)((a.waves + GTT_WAVES - 1) / GTT_WAVES));
    hipLaunchKernelGGL(k_gtt_moments, cell_grid, dim3(GTT_THREADS), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (disparity) {
        if ((e = gtt_launch_mode(r->d_disparity_u16, a.s.disp, n, Hs, Ws, stream)) != hipSuccess) return e;
        hipLaunchKernelGGL(k_gtt_hist, cell_grid, dim3(GTT_THREADS), 0, stream, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_gtt_median, dim3((unsigned)((capacity + GTT_WAVES - 1) / GTT_WAVES), (unsigned)n),
                           dim3(GTT_THREADS), 0, stream, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const int tile_rows = r->d_segmentation ? r->rows_power2_segmentation : Hs;
    hipLaunchKernelGGL(k_gtt_emit, dim3((unsigned)((Ws + GTT_TILE - 1) / GTT_TILE),
                                        (unsigned)((tile_rows + GTT_TILE - 1) / GTT_TILE), (unsigned)n),
                       dim3(GTT_THREADS), 0, stream, a);
    return hipGetLastError();
}

} /* extern "C" */
