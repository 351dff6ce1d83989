/*
 * is_k_assign_gt.hip -- f8: the instance id of every stixel from the GROUND-TRUTH instance image, by majority vote
 * over the stixel's rectangle (is_assign_instances_gt of instance_stixels_core.h).  It replaces the per-stixel
 * bincount loop of the reference tooling (tools/visualization/clustering_visualization.py assign_instances_gt
 * :846-891 over cityscapes_instance_loader.py load_instance_mask :32-71); the numpy restatement is
 * tests/assign_gt_reference.py.  The output is the per-section map that is_render_sections, is_instance_overlap and
 * is_stixel_world read, so the upper-bound rows of the instance evaluation never leave the device.
 *
 * One wave per (frame, stixel column), four adjacent columns per workgroup: at w == 8 the four 32-byte row pieces
 * of a workgroup's columns are one 128-byte line.  The wave takes its column's sections 64 at a time, one header
 * per lane; a ballot finds the terminator and the sections of an instance class (11..18), and only those touch the
 * ground truth.  For such a section the lanes take the rectangle's rows 64 at a time (w == 8, 8-pixel aligned rows:
 * two 16-byte loads per row, else pixel by pixel), tally runs of equal votes in registers and add them into the
 * wave's LDS histogram: bin 0 = background, bin 1 + k = instance k of the section's class, 1024 bins of which 1001
 * are used.  The lanes then scan the bins interleaved (lane l: l, l + 64, ...; conflict-free), clearing what they
 * read; a wave reduction picks the largest count, the smaller bin on a tie (bincount().argmax()).  Lane 0 applies
 * the minimum-fraction rule in binary64 and the result lands in the register of the lane that owns the section, so
 * the map is written once, 64 consecutive slots per store.  No global atomics, no allocation, no synchronisation.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "instance_stixels_core.h"
#include "is_launch.h"

#define IS_AGT_WAVES 4      /* waves = stixel columns per workgroup */
#define IS_AGT_BINS 1024    /* per wave: background + 1000 instance numbers, padded to 16 bins per lane */

struct AssignGtArgs {
    const is_section* sections;
    const int32_t* gt;
    int32_t* section_instance;
    int32_t* section_votes; /* may be null */
    int realcols, S, rows, cols, w, col_groups;
    double min_w;           /* min_fraction * w, the first product of the rule */
    int label_ids[IS_INSTANCE_CLASSES];
};

/* the bin of one ground-truth pixel for a section whose class owns [lo, lo + 1000) */
__device__ __forceinline__ int agt_bin(int v, int lo) {
    const unsigned k = (unsigned)v - (unsigned)lo; /* v in [lo, lo + 1000)  <=>  k < 1000 */
    return (v > 1000 && k < 1000u) ? 1 + (int)k : 0;
}

__device__ __forceinline__ void agt_add(unsigned* bins, int& key, unsigned& run, int b) {
    if (b == key) {
        run++;
        return;
    }
    if (run) atomicAdd(&bins[key], run);
    key = b;
    run = 1;
}

__device__ __forceinline__ void agt_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

/* VEC: w == 8, cols % 8 == 0 and a 16-byte aligned image: a row of the rectangle is two 16-byte loads */
template <bool VEC>
__global__ __launch_bounds__(64 * IS_AGT_WAVES) void k_assign_gt(const AssignGtArgs a) {
    __shared__ unsigned s_bins[IS_AGT_WAVES][IS_AGT_BINS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int f = blockIdx.x / a.col_groups;
    const int c = (blockIdx.x % a.col_groups) * IS_AGT_WAVES + wave;
    if (c >= a.realcols) return; /* (whole waves; the kernel has no workgroup barrier) */
    unsigned* const bins = s_bins[wave];
    for (int i = lane; i < IS_AGT_BINS; i += 64) bins[i] = 0;
    agt_wave_sync();

    const size_t column = ((size_t)f * a.realcols + c) * a.S;
    const is_section* const col = a.sections + column;
    const int32_t* const img = a.gt + (size_t)f * a.rows * a.cols + (size_t)c * a.w;
    bool open = true; /* no terminator so far */
    for (int base = 0; base < a.S; base += 64) {
        const int i = base + lane;
        int label = -1, votes = 0;
        int vB = 0, vT = 0, cls = 0;
        bool term = false;
        if (open && i < a.S) {
            const int4 h = *(const int4*)&col[i]; /* type, vB, vT, disparity */
            term = h.x == -1;
            vB = h.y;
            vT = h.z;
            cls = col[i].semantic_class;
        }
        uint64_t todo = 0;
        if (open) {
            const uint64_t terms = __ballot(term);
            const uint64_t front = terms ? (terms & (0 - terms)) - 1 : ~0ull; /* lanes in front of the terminator */
            todo = __ballot(i < a.S && cls >= IS_FIRST_INSTANCE_CLASS &&
                            cls < IS_FIRST_INSTANCE_CLASS + IS_INSTANCE_CLASSES) & front;
            if (terms) open = false;
        }
        while (todo) {
            const int src = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int sB = __shfl(vB, src, 64), sT = __shfl(vT, src, 64), sC = __shfl(cls, src, 64);
            const int lo = a.label_ids[sC - IS_FIRST_INSTANCE_CLASS] * 1000;
            /* rows [rows-1-vT, rows-1-vB] of the image, clipped to the frame (64-bit: hostile vB / vT) */
            const long long top = max((long long)a.rows - 1 - sT, 0ll);
            const long long bot = min((long long)a.rows - 1 - sB, (long long)a.rows - 1);
            if (top > bot) continue; /* an empty rectangle: -1, no vote */
            int key = 0;
            unsigned run = 0;
            for (int y = (int)top + lane; y <= (int)bot; y += 64) {
                const int32_t* const row = img + (size_t)y * a.cols;
                if (VEC) {
                    const int4 p = ((const int4*)row)[0], q = ((const int4*)row)[1];
                    agt_add(bins, key, run, agt_bin(p.x, lo));
                    agt_add(bins, key, run, agt_bin(p.y, lo));
                    agt_add(bins, key, run, agt_bin(p.z, lo));
                    agt_add(bins, key, run, agt_bin(p.w, lo));
                    agt_add(bins, key, run, agt_bin(q.x, lo));
                    agt_add(bins, key, run, agt_bin(q.y, lo));
                    agt_add(bins, key, run, agt_bin(q.z, lo));
                    agt_add(bins, key, run, agt_bin(q.w, lo));
                } else {
                    for (int k = 0; k < a.w; k++) agt_add(bins, key, run, agt_bin(row[k], lo));
                }
            }
            if (run) atomicAdd(&bins[key], run);
            agt_wave_sync();
            /* the largest count, the smaller bin on a tie: (count << 10 | 1023 - bin), maximised */
            unsigned long long best = 0;
            for (int j = 0; j < IS_AGT_BINS / 64; j++) {
                const int b = lane + 64 * j;
                const unsigned n = bins[b];
                if (n) {
                    bins[b] = 0;
                    const unsigned long long k = ((unsigned long long)n << 10) | (unsigned)(IS_AGT_BINS - 1 - b);
                    best = k > best ? k : best;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long other = __shfl_xor(best, o, 64);
                best = other > best ? other : best;
            }
            agt_wave_sync();
            const int win = IS_AGT_BINS - 1 - (int)(best & (IS_AGT_BINS - 1));
            const long long count = (long long)(best >> 10);
            /* the winner must NOT have fewer than (min_fraction * w) * (vT - vB) pixels (binary64, this order) */
            const bool few = (double)count < a.min_w * (double)((long long)sT - (long long)sB);
            if (lane == src) {
                votes = (int)count;
                label = (win > 0 && !few) ? win - 1 : -1;
            }
        }
        if (i < a.S) {
            a.section_instance[column + i] = label;
            if (a.section_votes) a.section_votes[column + i] = votes;
        }
    }
}

/* The labelled slots of a per-section map as (frame, column, section, label) quads behind a count, in no particular
 * order (the consumer builds a map from them): one atomic per wave for the positions, 16-byte stores. */
__global__ __launch_bounds__(256) void k_pack_section_labels(const int32_t* __restrict__ map, size_t n_slots,
                                                             int realcols, int S, int capacity, int32_t* packed) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int label = i < n_slots ? map[i] : -1;
    if (label < 0) return;
    const int at = atomicAdd(&packed[0], 1);
    if (at >= capacity) return;
    const size_t column = i / (size_t)S;
    ((int4*)packed)[1 + at] = make_int4((int)(column / (size_t)realcols), (int)(column % (size_t)realcols),
                                        (int)(i % (size_t)S), label);
}

extern "C" {

/* packed [4 + 4 * capacity], 16-byte aligned, packed[0] = 0 on entry */
hipError_t isk_launch_pack_section_labels(const int32_t* map, int n_images, int realcols, int max_sections,
                                          int capacity, int32_t* packed, hipStream_t stream) {
    const size_t n_slots = (size_t)n_images * realcols * max_sections;
    hipLaunchKernelGGL(k_pack_section_labels, dim3((unsigned)((n_slots + 255) / 256)), dim3(256), 0, stream, map,
                       n_slots, realcols, max_sections, capacity, packed);
    return hipGetLastError();
}

/* The arguments are checked by is_assign_instances_gt.  label_ids: the eight ids the kernel multiplies by 1000. */
hipError_t isk_launch_assign_gt(const is_assign_gt_args* r, const int* label_ids, hipStream_t stream) {
    AssignGtArgs a = {};
    a.sections = r->d_sections;
    a.gt = r->d_gt_instance;
    a.section_instance = r->d_section_instance;
    a.section_votes = r->d_section_votes;
    a.realcols = r->realcols;
    a.S = r->max_sections;
    a.rows = r->rows;
    a.cols = r->cols;
    a.w = r->cols / r->realcols;
    a.col_groups = (r->realcols + IS_AGT_WAVES - 1) / IS_AGT_WAVES;
    a.min_w = r->min_fraction * (double)a.w;
    for (int i = 0; i < IS_INSTANCE_CLASSES; i++) a.label_ids[i] = label_ids[i];
    const bool vec = a.w == 8 && a.cols % 8 == 0 && ((uintptr_t)a.gt & 15) == 0;
    const dim3 grid((unsigned)(r->n_images * a.col_groups));
    if (vec)
        hipLaunchKernelGGL(k_assign_gt<true>, grid, dim3(64 * IS_AGT_WAVES), 0, stream, a);
    else
        hipLaunchKernelGGL(k_assign_gt<false>, grid, dim3(64 * IS_AGT_WAVES), 0, stream, a);
    return hipGetLastError();
}

} /* extern "C" */
