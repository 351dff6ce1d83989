/*
 * is_conv_backward.h -- what the kernels of f21 (is_k_conv_backward.hip) and f22 (is_k_conv_backward_stride.hip) share:
 * the half roundings, the 32x32x16 MFMA of either half dtype and the LDS tile of the weight-gradient kernels.
 */
#ifndef IS_CONV_BACKWARD_H_
#define IS_CONV_BACKWARD_H_
#include "is_launch.h"

#define CB_SEG 32                  /* pixels of a staged segment: two K steps */
#define CB_TILE_ENTRIES 256        /* 16-byte entries of a 64-row x 32-pixel tile */

typedef float cb_acc __attribute__((ext_vector_type(16)));
typedef _Float16 cb_f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 cb_bf16x8 __attribute__((ext_vector_type(8)));

/* fp32 -> half, round to nearest even, as 16 bits (the rounding of is_conv_pack_weights) */
template <int DT> __device__ __forceinline__ uint16_t cb_round(float v);
template <> __device__ __forceinline__ uint16_t cb_round<IS_HEAD_F16>(float v) {
    return __builtin_bit_cast(uint16_t, (_Float16)v);
}
template <> __device__ __forceinline__ uint16_t cb_round<IS_HEAD_BF16>(float v) {
    const uint32_t u = __float_as_uint(v);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
/* half -> fp32, exact */
template <int DT> __device__ __forceinline__ float cb_widen(uint16_t u);
template <> __device__ __forceinline__ float cb_widen<IS_HEAD_F16>(uint16_t u) { return (float)__builtin_bit_cast(_Float16, u); }
template <> __device__ __forceinline__ float cb_widen<IS_HEAD_BF16>(uint16_t u) { return __uint_as_float((uint32_t)u << 16); }

template <int DT> __device__ __forceinline__ cb_acc cb_mfma(uint4 a, uint4 b, cb_acc c);
template <> __device__ __forceinline__ cb_acc cb_mfma<IS_HEAD_F16>(uint4 a, uint4 b, cb_acc c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(cb_f16x8, a), __builtin_bit_cast(cb_f16x8, b), c, 0, 0, 0);
}
template <> __device__ __forceinline__ cb_acc cb_mfma<IS_HEAD_BF16>(uint4 a, uint4 b, cb_acc c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(cb_bf16x8, a), __builtin_bit_cast(cb_bf16x8, b), c, 0, 0, 0);
}

/* entry of (slot s of 8 pixels, row) in a tile */
__device__ __forceinline__ int cb_entry(int s, int row) { return 64 * s + (row ^ (2 * s)); }

#endif /* IS_CONV_BACKWARD_H_ */
