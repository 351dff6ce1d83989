/* is_k_sweep.hip -- the small kernels of a parameter sweep (is_compute_sweep) and of the re-clustering
 * (is_recluster): everything else a sweep launches is the unchanged kernel of an ordinary call.
 *
 * The prepare launch of a sweep runs with disparity and instance weight 1 and the context's weight-free object slack
 * (is_core.hip, sweep_enqueue), so the PruneRec it leaves per column holds the slacks themselves:
 *   E1o = sigma_od, E1g = sig_g, E1s = sig_k, E2 = (2^-21 * safe) * sum      (1 * x is x),
 * or the explicit "off" state (every E1 = +inf) of a column whose pruning is off whatever the weights are: a generic
 * column, a wrapped offset channel, a slack that is not finite.  k_prune_scale writes each set's records from them.
 */
#include "is_dbscan.h"
#include "is_kernels.h"

#define SWP_THREADS 256

/* One lane per (set, column).  The expressions are those of the prepare launch (is_k_prepare.hip, "PruneRec"):
 * E1o / E1g / E1s are the same products of the same operands, bit for bit.  E2 is iw * (k * sum) where the prepare
 * launch computes (iw * k) * sum: the two differ by a rounding of 2^-24 relative, the factor safe = 1 + 2^-10 inside k
 * covers both, so the record still bounds the instance term.  A slack that is off in the base
 * is +inf or NaN there; the product with any weight is +inf or NaN again, and the tests below switch the set's record
 * off exactly as the prepare launch would have. */
__global__ __launch_bounds__(SWP_THREADS) void k_prune_scale(const PruneRec* __restrict__ base,
                                                             PruneRec* __restrict__ out, int ncols, int n_sets,
                                                             const SweepScale sc) {
    const int idx = (int)blockIdx.x * SWP_THREADS + (int)threadIdx.x;
    if (idx >= ncols * n_sets) return; /* (the host keeps ncols * IS_SWEEP_SCALE_SETS below 2^31) */
    const int set = idx / ncols, col = idx - set * ncols;
    const float4 s = *reinterpret_cast<const float4*>(base + col); /* sigma_od | sig_g | sig_k | E2 at iw = 1 */
    const float dw = sc.dw[set], iw = sc.iw[set], sigma_od = sc.sigma_od[set];
    float4 e;
    e.x = dw * sigma_od;
    e.y = dw * s.y;
    e.z = dw * s.z;
    e.w = iw * s.w;
    const bool base_off = !(s.x < IS_INF);
    if (base_off || !(sigma_od < IS_INF) || !(e.y < IS_INF) || !(e.z < IS_INF) || !(e.w < IS_INF))
        e.x = e.y = e.z = IS_INF;
    float4* o = reinterpret_cast<float4*>(out + (size_t)set * ncols + col);
    o[0] = e;
    o[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

/* The two words of a call that one DP consumes and a sweep needs once per set: the count of generic-encoding columns
 * (the prepare launch counts, block 0 of k_backtrace clears) and the walk's distrust word (the prepare launch clears,
 * a distrusted walk sets).  restore = 0, behind the prepare launch: the count is kept.  restore = 1, in front of every
 * set after the first: the count is put back and the distrust of the set before is forgotten. */
__global__ void k_sweep_state(int* __restrict__ n_generic, int* __restrict__ path_bad, int* __restrict__ saved,
                              int restore) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (restore) {
        *n_generic = *saved;
        path_bad[0] = 0;
    } else {
        *saved = *n_generic;
    }
}

/* One lane per candidate slot, grid = (chunks of the slots, 8 classes, n_images): the core-candidate flag of
 * k_compact_instances again (is_core_candidate, is_dbscan.h), from the candidate's (column, section index). */
__global__ __launch_bounds__(SWP_THREADS) void k_recore(int n_slots, int S, int size_filter,
                                                        const is_section* __restrict__ sections,
                                                        const is_instance_buffers* __restrict__ tbl) {
    const int cls = blockIdx.y, img = blockIdx.z;
    const is_instance_buffers ib = tbl[img];
    if (!ib.d_core_candidates || !ib.d_indices || !ib.d_instances_per_class) return;
    const int n = min(max(ib.d_instances_per_class[cls], 0), n_slots);
    const int i = (int)blockIdx.x * SWP_THREADS + (int)threadIdx.x;
    if (i >= n) return;
    const size_t o = (size_t)cls * n_slots + i;
    const int c = ib.d_indices[o * 2], si = ib.d_indices[o * 2 + 1];
    if (!IS_FRAME_SLOT(c, si, S, n_slots)) return;
    const is_section* s = sections + (size_t)img * n_slots + (size_t)c * S + si;
    ib.d_core_candidates[o] = is_core_candidate(s->vB, s->vT, size_filter);
}

extern "C" {

hipError_t isk_launch_prune_scale(const PruneRec* base, PruneRec* out, int ncols, int n_sets, const SweepScale* sc,
                                  hipStream_t stream) {
    const long long n = (long long)ncols * n_sets;
    hipLaunchKernelGGL(k_prune_scale, dim3((unsigned)((n + SWP_THREADS - 1) / SWP_THREADS)), dim3(SWP_THREADS), 0,
                       stream, base, out, ncols, n_sets, *sc);
    return hipGetLastError();
}

hipError_t isk_launch_sweep_state(int* n_generic, int* path_bad, int* saved, int restore, hipStream_t stream) {
    hipLaunchKernelGGL(k_sweep_state, dim3(1), dim3(64), 0, stream, n_generic, path_bad, saved, restore);
    return hipGetLastError();
}

hipError_t isk_launch_recore(int n_slots, int max_sections, int size_filter, int n_images, const is_section* sections,
                             const is_instance_buffers* d_tbl, hipStream_t stream) {
    hipLaunchKernelGGL(k_recore, dim3((n_slots + SWP_THREADS - 1) / SWP_THREADS, IS_INSTANCE_CLASSES, n_images),
                       dim3(SWP_THREADS), 0, stream, n_slots, max_sections, size_filter, sections, d_tbl);
    return hipGetLastError();
}

} /* extern "C" */
