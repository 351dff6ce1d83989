/*
 * is_k_objects.hip -- f9: the per-INSTANCE form of a batch (is_instance_objects of instance_stixels_core.h): one
 * 64-byte is_instance_object per (frame, class, label) that has a member stixel, and one 32-byte is_contour_point
 * per (object, stixel column holding a member) naming the depth-closest member of that column.  It is the keyed
 * reduction the reference's consumers do on the host over the per-stixel records (the top-down view and
 * draw_instance_masks of tools/visualization/clustering_visualization.py); the numpy restatement is
 * tests/objects_reference.py.
 *
 * The key space of a frame is dense: 8 classes x 1000 labels.  The scratch (stream-ordered allocator) holds per
 * frame a 32-byte accumulator per key, a bitmap of the stixel columns per key and, written by the finalize, the
 * (object index, first point) of every live key.  Every accumulator is stored so that zero is its identity (a
 * minimum as the maximum of the mirrored value), so one memset initialises the table.
 *   k_obj_columns<false>  wave per (frame, column): the headers 64 at a time, the map value beside them; a ballot
 *                         gives the terminator and the members.  Per distinct key of the column the lanes keep
 *                         partial sums / extremes over all rounds of the column and the wave reduces them once, so
 *                         ONE combine per (key, column) goes into the frame's table with device atomics -- integer
 *                         sums, integer maxima and a bit: the table does not depend on the order of arrival.
 *   k_obj_count           workgroup per frame: live keys and set column bits -> d_frame_objects, d_frame_points
 *   k_obj_emit            workgroup per frame: the frames in front of it summed, a scan of its keys in (class, label)
 *                         order, the object records as 16-byte stores, the (object, first point) of every live key,
 *                         the batch totals
 *   k_obj_columns<true>   the same walk again: the best member and the pixels of every (key, column); its place is
 *                         first_point + the number of set bits below the column in the key's bitmap; two lanes
 *                         write the point's two 16-byte chunks
 * The walk is done twice instead of staging a point per (key, column) between the passes: a frame's headers are a
 * few hundred kilobytes that stay in the L2, a staging buffer would be sized by the worst case.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "instance_stixels_core.h"
#include "is_launch.h"
#include "is_stixel_walk.h"

static_assert(sizeof(is_instance_object) == 64 && sizeof(is_contour_point) == 32 && sizeof(is_section) == 32,
              "the object kernels move 16-byte chunks");

#define IS_OBJ_KEYS (IS_INSTANCE_CLASSES * 1000) /* per frame: (class - 11) * 1000 + label */
#define IS_OBJ_WAVES 4                           /* waves = stixel columns per workgroup of the column walk */
#define IS_OBJ_THREADS 256                       /* of the per-frame kernels */
#define IS_OBJ_KEYS_PER_THREAD ((IS_OBJ_KEYS + IS_OBJ_THREADS - 1) / IS_OBJ_THREADS)

typedef unsigned long long u64;

/* The accumulator of one key.  top = max(rows - row), bottom = max(row + 1), dmax = max(ord(d)), dmin =
 * max(~ord(d)): zero is "nothing yet" for every field. */
struct ObjKey {
    unsigned n_stixels, pixels, top, bottom, dmax, dmin;
    u64 q16;
};
static_assert(sizeof(ObjKey) == 32, "one key is one 32-byte sector");

struct ObjArgs {
    const is_section* sections;
    const int32_t* map;
    ObjKey* keys;     /* [n][IS_OBJ_KEYS] */
    unsigned* bits;   /* [n][IS_OBJ_KEYS][words] */
    int2* slots;      /* [n][IS_OBJ_KEYS]: (object index, first point) of the live keys */
    is_instance_object* objects;
    is_contour_point* points;
    int32_t* frame_objects;
    int32_t* frame_points;
    int32_t* totals;
    int n_images, realcols, S, rows, w, words, object_capacity, point_capacity;
};

/* fp32 bits -> unsigned, monotone over the non-NaN floats (-0 below +0); 0 and ~0 are NaN patterns */
__device__ __forceinline__ unsigned obj_ord(unsigned bits) { return (bits & 0x80000000u) ? ~bits : bits | 0x80000000u; }
__device__ __forceinline__ unsigned obj_unord(unsigned o) { return (o & 0x80000000u) ? o & 0x7fffffffu : ~o; }

__device__ __forceinline__ unsigned obj_wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned obj_wave_max(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ u64 obj_wave_sum64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (u64)__shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ u64 obj_wave_max64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 other = (u64)__shfl_xor(v, o, 64);
        v = other > v ? other : v;
    }
    return v;
}

/* One round of a column: lane's section i.  key = the dense key of a member in front of the terminator, else -1.
 * Returns the ballot of the terminators. */
__device__ __forceinline__ uint64_t obj_round(const ObjArgs& a, const int4* src, const int32_t* map, int i, int lane,
                                              int& key, int& vB, int& vT, unsigned& dbits) {
    key = -1;
    vB = vT = 0;
    dbits = 0;
    bool term = false;
    if (i < a.S) {
        const int4 lo = src[2 * i], hi = src[2 * i + 1]; /* type, vB, vT, disparity | class, ... */
        const int label = map[i];
        term = lo.x == -1;
        vB = lo.y;
        vT = lo.z;
        dbits = (unsigned)lo.w;
        const unsigned cls = (unsigned)(hi.x - IS_FIRST_INSTANCE_CLASS);
        if (cls < (unsigned)IS_INSTANCE_CLASSES && (unsigned)label < 1000u) key = (int)cls * 1000 + label;
    }
    const uint64_t terms = __ballot(term);
    const uint64_t front = terms ? (terms & (0 - terms)) - 1 : ~0ull; /* lanes in front of the terminator */
    if (!((front >> lane) & 1)) key = -1;
    return terms;
}

/* A lane's partial result for the key in hand, over the rounds of the column. */
struct ObjAcc {
    unsigned cnt, hsum, top, bottom, dmax, dmin; /* top / bottom / dmax / dmin in ObjKey's mirrored forms */
    u64 q, best;                                 /* best = ord(d) (0 for NaN) << 32 | ~section: the largest wins */
    int best_vB, best_vT;
    unsigned best_d;
};

template <bool POINTS>
__device__ __forceinline__ void obj_take(ObjAcc& acc, int rows, int i, int vB, int vT, unsigned dbits) {
    /* rows [rows-1-vT, rows-1-vB] of the image, clipped to the frame (64-bit: hostile vB / vT) */
    const long long t = max((long long)rows - 1 - vT, 0ll), b = min((long long)rows - 1 - vB, (long long)rows - 1);
    const unsigned h = t <= b ? (unsigned)(b - t + 1) : 0u;
    const bool nan = (dbits & 0x7fffffffu) > 0x7f800000u;
    const unsigned o = obj_ord(dbits);
    acc.hsum += h;
    if (POINTS) {
        const u64 k = ((u64)(nan ? 0u : o) << 32) | (unsigned)~(unsigned)i;
        if (k > acc.best) {
            acc.best = k;
            acc.best_vB = vB;
            acc.best_vT = vT;
            acc.best_d = dbits;
        }
    } else {
        acc.cnt++;
        if (h) {
            acc.top = max(acc.top, (unsigned)(rows - (int)t));
            acc.bottom = max(acc.bottom, (unsigned)((int)b + 1));
        }
        if (!nan) {
            acc.dmax = max(acc.dmax, o);
            acc.dmin = max(acc.dmin, ~o);
        }
        const float d = __uint_as_float(dbits);
        if (d >= 0.0f && d < 32768.0f) acc.q += (u64)h * (u64)llrint((double)d * 65536.0);
    }
}

/* Wave per (frame, stixel column).  POINTS = false: the column's combine per key into the frame's table;
 * true (after k_obj_emit): the column's contour points. */
template <bool POINTS>
__global__ __launch_bounds__(64 * IS_OBJ_WAVES) void k_obj_columns(const ObjArgs a) {
    __shared__ unsigned s_seen[IS_OBJ_WAVES][IS_OBJ_KEYS / 32]; /* the keys of the column already dealt with */
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int gcol = __builtin_amdgcn_readfirstlane(blockIdx.x * IS_OBJ_WAVES + wave);
    if (gcol >= a.n_images * a.realcols) return; /* (whole waves; the kernel has no workgroup barrier) */
    const int f = gcol / a.realcols, c = gcol - f * a.realcols;
    unsigned* const seen = s_seen[wave];
    for (int i = lane; i < IS_OBJ_KEYS / 32; i += 64) seen[i] = 0;
    isw_wave_sync();

    const int4* const src = reinterpret_cast<const int4*>(a.sections + (size_t)gcol * a.S);
    const int32_t* const map = a.map + (size_t)gcol * a.S;
    const size_t frame_key = (size_t)f * IS_OBJ_KEYS;
    for (int base = 0; base < a.S; base += 64) {
        int key, vB, vT;
        unsigned dbits;
        const uint64_t terms = obj_round(a, src, map, base + lane, lane, key, vB, vT, dbits);
        uint64_t todo = __ballot(key >= 0);
        while (todo) {
            const int K = __shfl(key, __builtin_ctzll(todo), 64);
            todo &= ~__ballot(key == K);
            if ((seen[K >> 5] >> (K & 31)) & 1) continue; /* taken in an earlier round, with this round's members */
            ObjAcc acc = {};
            if (key == K) obj_take<POINTS>(acc, a.rows, base + lane, vB, vT, dbits);
            if (!terms && base + 64 < a.S) { /* a long column: this key's members of the later rounds, now */
                for (int b2 = base + 64; b2 < a.S; b2 += 64) {
                    int key2, vB2, vT2;
                    unsigned dbits2;
                    const uint64_t terms2 = obj_round(a, src, map, b2 + lane, lane, key2, vB2, vT2, dbits2);
                    if (key2 == K) obj_take<POINTS>(acc, a.rows, b2 + lane, vB2, vT2, dbits2);
                    if (terms2) break;
                }
                if (lane == 0) seen[K >> 5] |= 1u << (K & 31);
                isw_wave_sync();
            }
            const unsigned pixels = obj_wave_sum(acc.hsum) * (unsigned)a.w;
            if (POINTS) {
                const u64 best = obj_wave_max64(acc.best);
                const int winner = __builtin_ctzll(__ballot(acc.best == best)); /* the section index makes it unique */
                const int best_vB = __shfl(acc.best_vB, winner, 64), best_vT = __shfl(acc.best_vT, winner, 64);
                const unsigned best_d = __shfl(acc.best_d, winner, 64);
                const int2 slot = a.slots[frame_key + K];
                /* the key's columns in front of this one */
                const unsigned* const bm = a.bits + (frame_key + K) * a.words;
                unsigned below = 0;
                for (int j = lane; j <= (c >> 5); j += 64) {
                    const unsigned word = bm[j];
                    below += __popc(j == (c >> 5) ? word & ((1u << (c & 31)) - 1u) : word);
                }
                const int at = slot.y + (int)obj_wave_sum(below);
                if (at < a.point_capacity && lane < 2) {
                    int4* const out = reinterpret_cast<int4*>(a.points + at);
                    out[lane] = lane == 0 ? make_int4(slot.x, c, (int)~(unsigned)(best & 0xffffffffu), best_vB)
                                          : make_int4(best_vT, (int)pixels, (int)best_d, 0);
                }
            } else {
                const unsigned cnt = obj_wave_sum(acc.cnt);
                const unsigned top = obj_wave_max(acc.top), bottom = obj_wave_max(acc.bottom);
                const unsigned dmax = obj_wave_max(acc.dmax), dmin = obj_wave_max(acc.dmin);
                const u64 q = obj_wave_sum64(acc.q);
                ObjKey* const r = a.keys + frame_key + K;
                /* one update per field, a lane each */
                if (lane == 0) atomicAdd(&r->n_stixels, cnt);
                if (lane == 1 && pixels) atomicAdd(&r->pixels, pixels);
                if (lane == 2 && top) atomicMax(&r->top, top);
                if (lane == 3 && bottom) atomicMax(&r->bottom, bottom);
                if (lane == 4 && dmax) atomicMax(&r->dmax, dmax);
                if (lane == 5 && dmin) atomicMax(&r->dmin, dmin);
                if (lane == 6 && q) atomicAdd(&r->q16, q);
                if (lane == 7) atomicOr(&a.bits[(frame_key + K) * a.words + (c >> 5)], 1u << (c & 31));
            }
        }
        if (terms) break;
    }
}

/* the live keys of a thread (IS_OBJ_KEYS_PER_THREAD consecutive ones) and the set column bits of those */
__device__ __forceinline__ void obj_thread_counts(const ObjArgs& a, int f, int& live, int& cols) {
    live = cols = 0;
    const size_t frame_key = (size_t)f * IS_OBJ_KEYS;
    for (int j = 0; j < IS_OBJ_KEYS_PER_THREAD; j++) {
        const int K = threadIdx.x * IS_OBJ_KEYS_PER_THREAD + j;
        if (K >= IS_OBJ_KEYS || a.keys[frame_key + K].n_stixels == 0) continue;
        live++;
        const unsigned* const bm = a.bits + (frame_key + K) * a.words;
        for (int k = 0; k < a.words; k++) cols += __popc(bm[k]);
    }
}

/* Sum of (x, y) over the workgroup, and the exclusive prefix of this thread, threads in order. */
__device__ __forceinline__ void obj_block_scan(int x, int y, int2* s_wave, int2& before, int2& total) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int ix = x, iy = y; /* inclusive inside the wave */
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int ux = __shfl_up(ix, o, 64), uy = __shfl_up(iy, o, 64);
        if (lane >= o) {
            ix += ux;
            iy += uy;
        }
    }
    __syncthreads(); /* (s_wave may still be read from an earlier call) */
    if (lane == 63) s_wave[wave] = make_int2(ix, iy);
    __syncthreads();
    before = make_int2(ix - x, iy - y);
    total = make_int2(0, 0);
    for (int k = 0; k < IS_OBJ_THREADS / 64; k++) {
        const int2 t = s_wave[k];
        if (k < wave) {
            before.x += t.x;
            before.y += t.y;
        }
        total.x += t.x;
        total.y += t.y;
    }
}

__global__ __launch_bounds__(IS_OBJ_THREADS) void k_obj_count(const ObjArgs a) {
    __shared__ int2 s_wave[IS_OBJ_THREADS / 64];
    const int f = blockIdx.x;
    int live, cols;
    obj_thread_counts(a, f, live, cols);
    int2 before, total;
    obj_block_scan(live, cols, s_wave, before, total);
    if (threadIdx.x == 0) {
        a.frame_objects[f] = total.x;
        a.frame_points[f] = total.y;
    }
}

__global__ __launch_bounds__(IS_OBJ_THREADS) void k_obj_emit(const ObjArgs a) {
    __shared__ int2 s_wave[IS_OBJ_THREADS / 64];
    const int f = blockIdx.x;
    /* the objects and points of the frames in front of this one */
    int ox = 0, oy = 0;
    for (int g = threadIdx.x; g < f; g += IS_OBJ_THREADS) {
        ox += a.frame_objects[g];
        oy += a.frame_points[g];
    }
    int2 unused, base;
    obj_block_scan(ox, oy, s_wave, unused, base);
    int live, cols;
    obj_thread_counts(a, f, live, cols);
    int2 before, total;
    obj_block_scan(live, cols, s_wave, before, total);
    if (f == a.n_images - 1 && threadIdx.x == 0) {
        a.totals[0] = base.x + total.x;
        a.totals[1] = base.y + total.y;
    }
    int object = base.x + before.x, first_point = base.y + before.y;
    const size_t frame_key = (size_t)f * IS_OBJ_KEYS;
    for (int j = 0; j < IS_OBJ_KEYS_PER_THREAD && live > 0; j++) {
        const int K = threadIdx.x * IS_OBJ_KEYS_PER_THREAD + j;
        if (K >= IS_OBJ_KEYS) break;
        const ObjKey r = a.keys[frame_key + K];
        if (r.n_stixels == 0) continue;
        const unsigned* const bm = a.bits + (frame_key + K) * a.words;
        int n_columns = 0, col_min = -1, col_max = -1;
        for (int k = 0; k < a.words; k++) {
            const unsigned word = bm[k];
            if (!word) continue;
            if (col_min < 0) col_min = 32 * k + __builtin_ctz(word);
            col_max = 32 * k + 31 - __builtin_clz(word);
            n_columns += __popc(word);
        }
        a.slots[frame_key + K] = make_int2(object, first_point);
        if (object < a.object_capacity) {
            int4* const out = reinterpret_cast<int4*>(a.objects + object);
            out[0] = make_int4(f, IS_FIRST_INSTANCE_CLASS + K / 1000, K % 1000, (int)r.n_stixels);
            out[1] = make_int4(n_columns, first_point, (int)r.pixels, col_min);
            out[2] = make_int4(col_max, a.rows - (int)r.top, (int)r.bottom - 1, 0);
            out[3] = make_int4((int)(r.dmin ? obj_unord(~r.dmin) : 0x7f800000u),
                               (int)(r.dmax ? obj_unord(r.dmax) : 0xff800000u), (int)(unsigned)(r.q16 & 0xffffffffu),
                               (int)(unsigned)(r.q16 >> 32));
        }
        object++;
        first_point += n_columns;
        live--;
    }
}

extern "C" {

/* The arguments are checked by is_instance_objects. */
hipError_t isk_launch_instance_objects(const is_instance_objects_args* r, hipStream_t stream) {
    const int n = r->n_images;
    hipError_t e;
    if (!r->d_section_instance) { /* no map: no section is a member */
        if ((e = hipMemsetAsync(r->d_frame_objects, 0, sizeof(int32_t) * n, stream)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(r->d_frame_points, 0, sizeof(int32_t) * n, stream)) != hipSuccess) return e;
        return hipMemsetAsync(r->d_totals, 0, 2 * sizeof(int32_t), stream);
    }
    ObjArgs a = {};
    a.words = (r->realcols + 31) / 32;
    const size_t n_keys = (size_t)n * IS_OBJ_KEYS;
    const size_t zeros = n_keys * (sizeof(ObjKey) + sizeof(unsigned) * a.words);
    void* scratch = nullptr;
    if ((e = hipMallocAsync(&scratch, zeros + n_keys * sizeof(int2), stream)) != hipSuccess) return e;
    a.sections = r->d_sections;
    a.map = r->d_section_instance;
    a.keys = (ObjKey*)scratch;
    a.bits = (unsigned*)(a.keys + n_keys);
    a.slots = (int2*)((char*)scratch + zeros);
    a.objects = r->d_objects;
    a.points = r->d_points;
    a.frame_objects = r->d_frame_objects;
    a.frame_points = r->d_frame_points;
    a.totals = r->d_totals;
    a.n_images = n;
    a.realcols = r->realcols;
    a.S = r->max_sections;
    a.rows = r->rows;
    a.w = r->cols / r->realcols;
    a.object_capacity = r->object_capacity;
    a.point_capacity = r->point_capacity;
    e = hipMemsetAsync(scratch, 0, zeros, stream);
    if (e == hipSuccess) {
        const dim3 columns((unsigned)((n * r->realcols + IS_OBJ_WAVES - 1) / IS_OBJ_WAVES));
        hipLaunchKernelGGL(k_obj_columns<false>, columns, dim3(64 * IS_OBJ_WAVES), 0, stream, a);
        hipLaunchKernelGGL(k_obj_count, dim3(n), dim3(IS_OBJ_THREADS), 0, stream, a);
        hipLaunchKernelGGL(k_obj_emit, dim3(n), dim3(IS_OBJ_THREADS), 0, stream, a);
        hipLaunchKernelGGL(k_obj_columns<true>, columns, dim3(64 * IS_OBJ_WAVES), 0, stream, a);
        e = hipGetLastError();
    }
    const hipError_t e2 = hipFreeAsync(scratch, stream);
    return e == hipSuccess ? e2 : e;
}

} /* extern "C" */
