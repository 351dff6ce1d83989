/*
 * is_k_assign_gt.hip -- f8: the instance id of every stixel from the GROUND-TRUTH instance image, by majority vote
 * over the stixel's rectangle (is_assign_instances_gt of instance_stixels_core.h).  It replaces the per-stixel
 * bincount loop of the reference tooling (tools/visualization/clustering_visualization.py assign_instances_gt
 * :846-891 over cityscapes_instance_loader.py load_instance_mask :32-71); the numpy restatement is
 * tests/assign_gt_reference.py.  The output is the per-section map that is_render_sections, is_instance_overlap and
 * is_stixel_world read, so the upper-bound rows of the instance evaluation never leave the device.
 *
 * One wave per (frame, stixel column), four adjacent columns per workgroup: at w == 8 the four 32-byte row pieces
 * of a workgroup's columns are one 128-byte line.  The walk over the column's sections and their pixels is
 * is_stixel_walk.h; the wave's LDS histogram has bin 0 = background, bin 1 + k = instance k of the section's class,
 * 1024 bins of which 1001 are used.  The lanes then scan the bins interleaved (lane l: l, l + 64, ...; conflict-free),
 * clearing what they read; a wave reduction picks the largest count, the smaller bin on a tie (bincount().argmax()).
 * Lane 0 applies the minimum-fraction rule in binary64 and the result lands in the register of the lane that owns the
 * section, so the map is written once, 64 consecutive slots per store.  No global atomics, no allocation, no
 * synchronisation.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "instance_stixels_core.h"
#include "is_launch.h"
#include "is_stixel_walk.h"

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
__device__ __forceinline__ unsigned agt_bin(int v, int lo) {
    const unsigned k = (unsigned)v - (unsigned)lo; /* v in [lo, lo + 1000)  <=>  k < 1000 */
    return (v > 1000 && k < 1000u) ? 1u + k : 0u;
}

/* VEC: as isw_tally */
template <bool VEC>
__global__ __launch_bounds__(64 * IS_AGT_WAVES) void k_assign_gt(const AssignGtArgs a) {
    __shared__ unsigned s_bins[IS_AGT_WAVES][IS_AGT_BINS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int f = blockIdx.x / a.col_groups;
    const int c = (blockIdx.x % a.col_groups) * IS_AGT_WAVES + wave;
    if (c >= a.realcols) return; /* (whole waves; the kernel has no workgroup barrier) */
    unsigned* const bins = s_bins[wave];
    for (int i = lane; i < IS_AGT_BINS; i += 64) bins[i] = 0;
    isw_wave_sync();

    const size_t column = ((size_t)f * a.realcols + c) * a.S;
    const is_section* const col = a.sections + column;
    const int32_t* const img = a.gt + (size_t)f * a.rows * a.cols + (size_t)c * a.w;
    bool open = true; /* no terminator so far */
    for (int base = 0; base < a.S; base += 64) {
        const int i = base + lane;
        int label = -1, votes = 0;
        int vB, vT, cls;
        uint64_t todo = isw_round(col, i, a.S, open, vB, vT, cls);
        while (todo) {
            const int src = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int sB = __shfl(vB, src, 64), sT = __shfl(vT, src, 64), sC = __shfl(cls, src, 64);
            const int lo = a.label_ids[sC - IS_FIRST_INSTANCE_CLASS] * 1000;
            const auto bin = [lo](int v) { return agt_bin(v, lo); };
            if (!isw_tally<VEC, 0>(img, a.rows, a.cols, a.w, sB, sT, lane, bins, bin)) continue; /* empty: no vote */
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
            isw_wave_sync();
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
