/* is_k_cluster.hip -- size-filtered DBSCAN over the predicted instance centres: the rules, the body and
 * the packed emit are is_dbscan.h, over the two coordinates of a centre.  One workgroup per (image, instance class),
 * and a batch is ONE launch: grid = (8 classes, n_images).  Nothing leaves the device: Stixels::Compute does not copy
 * candidates to the host to cluster them.
 */
#include "is_dbscan.h"
#include "is_kernels.h"

__device__ __forceinline__ void cluster_class(int n, float eps2, int min_pts, const dbs_f2* com,
                                              const uint8_t* cand, int32_t* const labels_out, int32_t* rank,
                                              int32_t* out, int* s_red, dbs_f2* s_com, uint8_t* s_cand,
                                              int32_t* s_lab) {
    const int tid = threadIdx.x;
    if (n == 0) return;
    /* The sweeps read centre, flag and component of EVERY candidate j for every candidate i: the
     * same address in all lanes, one dependent L2 round trip per j when the arrays lie in global
     * memory (a class of 300 candidates: 85 us).  Up to DBS_LDS_N candidates the three arrays are
     * copied into LDS first. */
    if (n <= DBS_LDS_N) {
        for (int i = tid; i < n; i += DBS_THREADS) { s_com[i] = com[i]; s_cand[i] = cand[i]; }
        __syncthreads();
        dbs_body(n, eps2, min_pts, dbs_points2<const lds_float2*>{(const lds_float2*)s_com}, (const lds_u8*)s_cand,
                 (lds_i32*)s_lab, labels_out, rank, out, s_red);
    } else {
        dbs_body(n, eps2, min_pts, dbs_points2<const dbs_f2*>{com}, cand, labels_out, labels_out, rank, out, s_red);
    }
}

/* One workgroup per (instance class, image): grid = (8, n_images).  `tbl[image]` holds the
 * image's candidate arrays (NULL: the single image `one`); images without d_labels are skipped.
 * `packed` (optional, per image): the triples of DBS_EMIT_PACKED -- everything Stixels::GetInstanceStixels needs in one
 * small copy.  scratch: [n_images][classes][2][n_slots]. */
__global__ __launch_bounds__(DBS_THREADS) void k_cluster_instances(
    int n_slots, float eps2, int min_pts, const is_instance_buffers* __restrict__ tbl,
    const is_instance_buffers one, int32_t* __restrict__ scratch) {
    __shared__ int s_red[DBS_THREADS];
    __shared__ dbs_f2 s_com[DBS_LDS_N];
    __shared__ int32_t s_lab[DBS_LDS_N];
    __shared__ uint8_t s_cand[DBS_LDS_N];
    const int cls = blockIdx.x, img = blockIdx.y;
    const is_instance_buffers ib = tbl ? tbl[img] : one;
    if (!ib.d_labels) return;
    const int32_t* per_class = ib.d_instances_per_class;
    const int n = dbs_class_count(per_class, cls, n_slots);
    const dbs_f2* com = reinterpret_cast<const dbs_f2*>(ib.d_centerofmass) + (size_t)cls * n_slots;
    const uint8_t* cand = ib.d_core_candidates + (size_t)cls * n_slots;
    int32_t* labels = ib.d_labels + (size_t)cls * n_slots;
    int32_t* rank = scratch + ((size_t)img * IS_INSTANCE_CLASSES + cls) * 2 * n_slots;
    cluster_class(n, eps2, min_pts, com, cand, labels, rank, rank + n_slots, s_red, s_com, s_cand, s_lab);
    int32_t* packed = ib.d_packed;
    if (packed && ib.d_indices) {
        __syncthreads();
        int base = 0, total = 0;
        DBS_CLASS_RANGE(per_class, cls, n_slots, base, total);
        DBS_EMIT_PACKED(packed, cls, n, base, total, ib.d_indices + (size_t)cls * n_slots * 2, labels);
    }
}

extern "C" hipError_t isk_launch_cluster(int n_slots, float eps, int min_pts, int n_images,
                                         const is_instance_buffers* d_tbl,
                                         const is_instance_buffers* one, int32_t* scratch,
                                         hipStream_t stream) {
    is_instance_buffers o;
    if (one) o = *one; else o = is_instance_buffers{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(k_cluster_instances, dim3(IS_INSTANCE_CLASSES, n_images), dim3(DBS_THREADS), 0,
                       stream, n_slots, eps * eps, min_pts, d_tbl, o, scratch);
    return hipGetLastError();
}
