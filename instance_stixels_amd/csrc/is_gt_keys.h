/*
 * is_gt_keys.h -- the parts that the keyed reductions over ground-truth instance ids share (is_k_gt_targets.hip, f11,
 * and is_k_offset_loss.hip, f12): a frame's open-addressing table of its keys (ids > 1000), the runs of equal tags
 * along a wave, and the lower median of a key's histogram of q = uint16 / 256.  Integer atomics only.
 */
#ifndef IS_GT_KEYS_H
#define IS_GT_KEYS_H

#include <hip/hip_runtime.h>

#include <stdint.h>

#define GTT_BINS 256 /* q = uint16 / 256 */

/* One slot of a frame's table; key 0 = free (a key is > 1000). */
struct GttEntry {
    int key;
    unsigned n;
    unsigned long long sy, sx;
    int number; /* the key's number in order of arrival: its histogram (f11) */
    int rank;   /* f12: the keys of the frame below this one, an order that does not depend on the arrival */
};
static_assert(sizeof(GttEntry) == 32, "one table slot is 32 bytes");

static inline unsigned gtt_log_slots(size_t cells) {
    unsigned lg = 1; /* 2 * pow2(cells) */
    while (((size_t)1 << (lg - 1)) < cells) lg++;
    return lg;
}

__device__ __forceinline__ unsigned gtt_hash(int key, unsigned log_slots) {
    return ((unsigned)key * 2654435761u) >> (32 - log_slots);
}

/* The slot of a key that was entered by an earlier launch; NULL cannot happen for such a key, the table is never
 * full and the walk ends at a free slot. */
__device__ __forceinline__ const GttEntry* gtt_find(const GttEntry* table, unsigned log_slots, int key) {
    const unsigned mask = (1u << log_slots) - 1u;
    unsigned at = gtt_hash(key, log_slots);
    for (;;) {
        const int k = table[at].key;
        if (k == key) return &table[at];
        if (k == 0) return nullptr;
        at = (at + 1) & mask;
    }
}

/* Enters `key` into the frame's table if it is new and returns its slot.  The lane that claims the slot numbers the
 * key with the frame's count so far: `fresh` is that number, -1 for a key that was there.  Ends: a frame has no more
 * keys than cells, and the table has twice as many slots. */
__device__ __forceinline__ unsigned gtt_enter(GttEntry* table, unsigned log_slots, int key, int32_t* count,
                                              int& fresh) {
    const unsigned mask = (1u << log_slots) - 1u;
    unsigned at = gtt_hash(key, log_slots);
    fresh = -1;
    for (;;) {
        const int k = atomicCAS(&table[at].key, 0, key);
        if (k == 0) {
            fresh = atomicAdd(count, 1);
            table[at].number = fresh;
            break;
        }
        if (k == key) break;
        at = (at + 1) & mask;
    }
    return at;
}

/* The runs of equal `tag` (0: none) along the wave's lanes: true in the first lane of a run with a tag, `next` the
 * lane behind the run's last. */
__device__ __forceinline__ bool gtt_run_head(bool differs, bool tagged, int lane, int& next) {
    const uint64_t starts = __ballot(lane == 0 || differs);
    const uint64_t above = lane == 63 ? 0 : starts >> (lane + 1);
    next = above ? lane + 1 + __builtin_ctzll(above) : 64;
    return tagged && ((starts >> lane) & 1);
}

/* A whole wave on one histogram of GTT_BINS counts (bin 0 is never added to): N = its total, and the bin of rank
 * (N - 1) / 2, the lower of the middle pair (torch.median); 0 where N is 0. */
__device__ __forceinline__ int gtt_lower_median(const unsigned* hist, int lane, unsigned& N) {
    const uint4 c = ((const uint4*)hist)[lane];
    const unsigned sum = c.x + c.y + c.z + c.w;
    unsigned incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    N = __shfl(incl, 63, 64);
    int median = 0;
    if (N) {
        const unsigned r = (N - 1) / 2, excl = incl - sum, rr = r - excl;
        const bool hit = excl <= r && r < incl;
        const int bin = 4 * lane + (rr < c.x ? 0 : rr < c.x + c.y ? 1 : rr < c.x + c.y + c.z ? 2 : 3);
        median = __shfl(bin, __builtin_ctzll(__ballot(hit)), 64);
    }
    return median;
}

#endif /* IS_GT_KEYS_H */
