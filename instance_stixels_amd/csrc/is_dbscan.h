/*
 * is_dbscan.h -- the size-filtered DBSCAN over instance candidates, once: k_cluster_instances (is_k_cluster.hip,
 * SURVEY f1) runs it over two coordinates, k_idisp_cluster (is_k_instance_disparity.hip, f10) over three and a
 * participation mask.  Also the class ranges, the packed emit and the core-candidate flag the cluster kernels share.
 *
 * The reference calls `ML::dbscanFit` of a cuML fork whose source is not in its tree
 * (/root/reference/InstanceStixels/src/Stixels.cu:639-681; branch `dbscan-sizefilter`, no commit
 * pinned, singularity_recipe:108-110).  The semantics built here are those of its Python twin
 * (/root/reference/tools/visualization/clustering_visualization.py:894-960):
 *
 *   large = candidates with height >= size_filter (the core-candidate flag written by the
 *           back-trace, StixelsKernels.cu:940-941); nothing is labelled unless
 *           #large > min_pts (:926);
 *   DBSCAN(eps, min_samples = min_pts) over the large points only (:928-929): a large point is a
 *           core point when >= min_pts large points (itself included) lie within eps; core
 *           points within eps of each other share a cluster; clusters are numbered in the order
 *           of their first core point; a large non-core point takes the cluster that reaches it
 *           first (= the lowest-numbered one among its core neighbours) or -1;
 *   every small point takes the label of its NEAREST core point if that lies within eps, else
 *           -1 (:935-948; first core on ties).
 *   A point set that can exclude points (PTS::MASKED, the three-coordinate one: a stixel median of 0) keeps them out
 *           of all of the above: never large, core, neighbour or nearest-core target; label -1.
 *
 * Distances: fp32, dx*dx + dy*dy (+ dz*dz), summed left to right and compared with eps*eps (no contraction), like
 * cuML on float input.  One workgroup of DBS_THREADS per (image, instance class); N <= realcols * max_sections, in
 * practice a few hundred, so the O(N^2) neighbour sweeps are a few microseconds and nothing leaves the device.
 */
#ifndef IS_DBSCAN_H_
#define IS_DBSCAN_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "instance_stixels_core.h"

#define DBS_THREADS 256
#define DBS_LDS_N 2048 /* classes with up to this many candidates are clustered out of LDS copies */

/* LDS pointer types: with them the sweeps compile to ds_read (pipelined, unrolled) instead of flat loads */
typedef float dbs_f2 __attribute__((ext_vector_type(2))); /* (a builtin vector: loadable from any address space) */
typedef __attribute__((address_space(3))) dbs_f2 lds_float2;
typedef __attribute__((address_space(3))) float lds_float;
typedef __attribute__((address_space(3))) uint8_t lds_u8;
typedef __attribute__((address_space(3))) int32_t lds_i32;

/* ---- the core-candidate flag ("large") of a section, and the guard of the kernels that derive it again from a
 * candidate's (column, section index): is that an index of a frame of n_slots = realcols * S sections?  (The guard is
 * a macro so that its tests short-circuit inside the caller's `if`: the code k_recore is held to.) ---- */
__device__ __forceinline__ bool is_core_candidate(int vB, int vT, int size_filter) {
    return (vT + 1 - vB) >= size_filter;
}
#define IS_FRAME_SLOT(c, si, S, n_slots) \
    ((c) >= 0 && (si) >= 0 && (si) < (S) && (size_t)(c) * (S) + (si) < (size_t)(n_slots))

/* ---- point sets: at(i), part(i) "takes part at all", d2(P, P); XY / Z point to global memory or to LDS copies ---- */
template <class XY>
struct dbs_points2 {
    static constexpr bool MASKED = false;
    typedef dbs_f2 P;
    XY xy;
    __device__ __forceinline__ P at(int i) const { return xy[i]; }
    __device__ __forceinline__ bool part(int) const { return true; }
    static __device__ __forceinline__ float d2(const P a, const P b) {
        const float dx = a.x - b.x, dy = a.y - b.y;
        return dx * dx + dy * dy;
    }
};

template <class XY, class Z>
struct dbs_points3 {
    static constexpr bool MASKED = true;
    struct P { dbs_f2 xy; float z; };
    XY xy;
    Z z;
    __device__ __forceinline__ P at(int i) const { return P{xy[i], z[i]}; }
    __device__ __forceinline__ bool part(int i) const { return z[i] != 0.0f; }
    static __device__ __forceinline__ float d2(const P a, const P b) {
        const float dx = a.xy.x - b.xy.x, dy = a.xy.y - b.xy.y, dz = a.z - b.z;
        return dx * dx + dy * dy + dz * dz;
    }
};

/* labels doubles as the component array while the kernel runs:
 *   >= 0  core point, value = smallest core index known to be in the same cluster
 *   -2    large, not core        -3   small        -4   (MASKED only) takes no part
 * pts / cand / labels: the points, large flags and component array -- global memory, or LDS copies (address_space(3)
 * types).  labels_out: the caller's array in global memory.  rank / out are scratch of n ints each, s_red of
 * DBS_THREADS ints.  Every thread of the workgroup calls it. */
template <class PTS, class CAND, class LAB>
__device__ __forceinline__ void dbs_body(int n, float eps2, int min_pts, const PTS pts, CAND cand, LAB labels,
                                         int32_t* const labels_out, int32_t* rank, int32_t* out, int* s_red) {
    typedef typename PTS::P P;
    const int tid = threadIdx.x;
    /* number of large points that take part: the twin clusters only if it exceeds min_pts (:926) */
    int cnt = 0;
    for (int i = tid; i < n; i += DBS_THREADS) cnt += cand[i] != 0 && (!PTS::MASKED || pts.part(i));
    s_red[tid] = cnt;
    __syncthreads();
    for (int s = DBS_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) s_red[tid] += s_red[tid + s];
        __syncthreads();
    }
    const int n_large = s_red[0];
    __syncthreads();
    if (n_large <= min_pts) {
        for (int i = tid; i < n; i += DBS_THREADS) labels_out[i] = -1;
        return;
    }

    /* core points */
    for (int i = tid; i < n; i += DBS_THREADS) {
        int l = (!PTS::MASKED || pts.part(i)) ? -3 : -4;
        if (l == -3 && cand[i]) {
            const P p = pts.at(i);
            int c = 0;
            for (int j = 0; j < n; j++)
                c += (cand[j] != 0) && (!PTS::MASKED || pts.part(j)) && (PTS::d2(p, pts.at(j)) <= eps2);
            l = (c >= min_pts) ? i : -2;
        }
        labels[i] = l;
    }
    __syncthreads();

    /* connected components of the core points: minimum-index propagation with pointer jumping;
     * labels only ever decrease, so reading a neighbour's value mid-update is harmless */
    for (;;) {
        int changed = 0;
        for (int i = tid; i < n; i += DBS_THREADS) {
            const int li = labels[i];
            if (li < 0) continue;
            const P p = pts.at(i);
            int m = li;
            for (int j = 0; j < n; j++) {
                const int lj = labels[j];
                if (lj >= 0 && lj < m && PTS::d2(p, pts.at(j)) <= eps2) m = lj;
            }
            while (labels[m] < m) m = labels[m]; /* jump to the current root */
            if (m < li) { labels[i] = m; changed = 1; }
        }
        if (!__syncthreads_or(changed)) break;
    }

    /* cluster number = rank of the root (smallest core index of the cluster) among the roots:
     * the order in which a scan over the points discovers the clusters */
    {
        const int per = (n + DBS_THREADS - 1) / DBS_THREADS;
        const int lo = tid * per, hi = min(lo + per, n); /* (lo > n: an empty range) */
        int c = 0;
        for (int i = lo; i < hi; i++) c += labels[i] == i;
        s_red[tid] = c;
        __syncthreads();
        int base = 0;
        for (int t = 0; t < tid; t++) base += s_red[t];
        for (int i = lo; i < hi; i++) {
            rank[i] = base;
            base += labels[i] == i;
        }
    }
    __syncthreads();

    for (int i = tid; i < n; i += DBS_THREADS) {
        const int li = labels[i];
        int res = -1;
        if (li >= 0) {
            res = rank[li];
        } else if (!PTS::MASKED || li != -4) {
            const P p = pts.at(i);
            if (li == -2) { /* border point: lowest-numbered cluster among the core neighbours */
                int best = n;
                for (int j = 0; j < n; j++) {
                    const int lj = labels[j];
                    if (lj >= 0 && lj < best && PTS::d2(p, pts.at(j)) <= eps2) best = lj;
                }
                if (best < n) res = rank[best];
            } else { /* small point: nearest core point, first one on ties, within eps */
                float bd = __builtin_inff();
                int bj = -1;
                for (int j = 0; j < n; j++) {
                    if (labels[j] < 0) continue;
                    const float d = PTS::d2(p, pts.at(j));
                    if (d < bd) { bd = d; bj = j; }
                }
                if (bj >= 0 && bd <= eps2) res = rank[labels[bj]];
            }
        }
        out[i] = res;
    }
    __syncthreads();
    for (int i = tid; i < n; i += DBS_THREADS) labels_out[i] = out[i];
}

/* The candidates of class k of a frame, and the two statements around the body that both cluster kernels hold -- as
 * macros: as inlined functions they reorder the once-per-workgroup tail of k_cluster_instances, whose code is held
 * instruction for instruction.  DBS_CLASS_RANGE adds to base the candidates of the classes in front of cls and to
 * total those of all classes: where the class's triples start in d_packed, and its first word.  DBS_EMIT_PACKED writes
 * packed[0] = total, then one (column, section index, label) triple per candidate, classes in ascending order: the
 * workgroup of class cls its n triples from `base` on.  idx / labels: the class's d_indices and (final) d_labels. */
__device__ __forceinline__ int dbs_class_count(const int32_t* per_class, int k, int n_slots) {
    return min(max(per_class[k], 0), n_slots);
}
#define DBS_CLASS_RANGE(per_class, cls, n_slots, base, total)               \
    for (int k_ = 0; k_ < IS_INSTANCE_CLASSES; k_++) {                      \
        const int m_ = dbs_class_count((per_class), k_, (n_slots));         \
        if (k_ < (cls)) (base) += m_;                                       \
        (total) += m_;                                                      \
    }
#define DBS_EMIT_PACKED(packed, cls, n, base, total, idx, labels)           \
    do {                                                                    \
        if ((cls) == 0 && threadIdx.x == 0) (packed)[0] = (total);          \
        const int32_t* const idx_ = (idx);                                  \
        for (int i_ = threadIdx.x; i_ < (n); i_ += DBS_THREADS) {           \
            int32_t* t_ = (packed) + 1 + (size_t)((base) + i_) * 3;         \
            t_[0] = idx_[2 * i_]; t_[1] = idx_[2 * i_ + 1]; t_[2] = (labels)[i_]; \
        }                                                                   \
    } while (0)

#endif /* IS_DBSCAN_H_ */
