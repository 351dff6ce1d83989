/*
 * is_stixel_walk.h -- the walk of one wave over one stixel column and the ground-truth pixels of its instance-class
 * sections, once: k_assign_gt (is_k_assign_gt.hip, a vote per section) and k_idisp_stixel
 * (is_k_instance_disparity.hip, a median per section) differ in how a pixel maps to a bin and in what they read out of
 * the bins afterwards.
 *
 * The wave takes its column's sections 64 at a time, one 16-byte header per lane (isw_round); a ballot finds the
 * terminator and the sections of an instance class (11..18) in front of it, and only those touch the ground truth.
 * For such a section the lanes take the rectangle's rows 64 at a time (VEC: two 16-byte loads per row, else pixel by
 * pixel), merge runs of equal bins in registers and add them into the wave's LDS histogram (isw_tally).  The kernels
 * have no workgroup barrier: a wave orders its own LDS traffic with isw_wave_sync.
 */
#ifndef IS_STIXEL_WALK_H_
#define IS_STIXEL_WALK_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "instance_stixels_core.h"

/* what a wave wrote to LDS is visible to its other lanes behind this */
__device__ __forceinline__ void isw_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

/* One round of a column: the lane's section i (vB, vT, class; 0 where there is none).  Returns the lanes whose section
 * is of an instance class and lies in front of the terminator; `open` (no terminator so far) is cleared by the round
 * that finds it, and a round of a closed column loads nothing and returns 0. */
__device__ __forceinline__ uint64_t isw_round(const is_section* col, int i, int S, bool& open, int& vB, int& vT,
                                              int& cls) {
    vB = vT = cls = 0;
    bool term = false;
    if (open && i < S) {
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
        todo = __ballot(i < S && cls >= IS_FIRST_INSTANCE_CLASS &&
                        cls < IS_FIRST_INSTANCE_CLASS + IS_INSTANCE_CLASSES) & front;
        if (terms) open = false;
    }
    return todo;
}

/* one more pixel of bin b for a lane's run (key, run); a finished run goes to the histogram unless its bin is below
 * MIN_BIN */
template <unsigned MIN_BIN>
__device__ __forceinline__ void isw_add(unsigned* bins, unsigned& key, unsigned& run, unsigned b) {
    if (b == key) {
        run++;
        return;
    }
    if (run && key >= MIN_BIN) atomicAdd(&bins[key], run);
    key = b;
    run = 1;
}

/* The pixels of the section (sB, sT) of a column of width w, whose first pixel of row 0 is img, into the wave's bins:
 * rows [rows-1-sT, rows-1-sB] of the image, clipped to the frame (64-bit: hostile vB / vT).  false: an empty
 * rectangle, nothing was touched.  bin_of_pixel(int ground-truth value) -> unsigned bin.  VEC: w == 8, cols % 8 == 0
 * and a 16-byte aligned image.  Every lane of the wave calls it; behind it the bins are complete. */
template <bool VEC, unsigned MIN_BIN, class BIN>
__device__ __forceinline__ bool isw_tally(const int32_t* img, int rows, int cols, int w, int sB, int sT, int lane,
                                          unsigned* bins, BIN bin_of_pixel) {
    const long long top = max((long long)rows - 1 - sT, 0ll);
    const long long bot = min((long long)rows - 1 - sB, (long long)rows - 1);
    if (top > bot) return false;
    unsigned key = 0, run = 0;
    for (int y = (int)top + lane; y <= (int)bot; y += 64) {
        const int32_t* const row = img + (size_t)y * cols;
        if (VEC) {
            const int4 p = ((const int4*)row)[0], q = ((const int4*)row)[1];
            const int v[8] = {p.x, p.y, p.z, p.w, q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 8; k++) isw_add<MIN_BIN>(bins, key, run, bin_of_pixel(v[k]));
        } else {
            for (int k = 0; k < w; k++) isw_add<MIN_BIN>(bins, key, run, bin_of_pixel(row[k]));
        }
    }
    if (run && key >= MIN_BIN) atomicAdd(&bins[key], run);
    isw_wave_sync();
    return true;
}

#endif /* IS_STIXEL_WALK_H_ */
