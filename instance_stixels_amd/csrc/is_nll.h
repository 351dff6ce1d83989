/*
 * is_nll.h -- what the two semantic NLL losses share: the record a workgroup leaves for the launch that joins them
 * and the tree that makes it, is_k_nll.hip (f14, is_semantic_nll) and is_k_nll_up.hip (f16, is_semantic_nll_up).
 * The joining launches are not shared: their summation orders differ, and each is its entry point's contract.
 */
#ifndef IS_NLL_H_
#define IS_NLL_H_

#include <hip/hip_runtime.h>

#define NLL_THREADS 256

/* a workgroup's pixels: the loss summed over the valid ones, their number, and the number of targets that are neither
 * a class nor ignore_index */
struct nll_partial {
    double sum;
    int valid, bad;
};
static_assert(sizeof(nll_partial) == 16, "one 16-byte record per workgroup");

/* s, v and b become their sums over the NLL_THREADS threads of a workgroup, in a fixed order: halves folded onto each
 * other.  sd, sv and sb are NLL_THREADS entries of LDS each. */
__device__ __forceinline__ void nll_tree(double& s, int& v, int& b, double* sd, int* sv, int* sb, int tid) {
    sd[tid] = s, sv[tid] = v, sb[tid] = b;
    __syncthreads();
    for (int step = NLL_THREADS / 2; step > 0; step >>= 1) {
        if (tid < step) sd[tid] += sd[tid + step], sv[tid] += sv[tid + step], sb[tid] += sb[tid + step];
        __syncthreads();
    }
    s = sd[0], v = sv[0], b = sb[0];
}

#endif /* IS_NLL_H_ */
