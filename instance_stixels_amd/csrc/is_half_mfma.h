/*
 * is_half_mfma.h -- the device vocabulary of the kernels that multiply half operands (fp16 or bf16, as 16 bits) with
 * MFMA into fp32: is_k_conv3x3.hip (f17-f19), is_k_stem.hip (f20), is_k_conv_backward.hip (f21),
 * is_k_conv_backward_stride.hip (f22) and is_k_stem_backward.hip (f23).  One copy of the roundings, the MFMA of either
 * dtype, the LDS slot swizzle, the C/D row map, the rounded scaled weight, and the launchers' dtype dispatch.
 *
 * Not here: HbFeature::narrow of is_k_head_backward.hip (and the head kernels' fp32 MFMA).  The head's contract keeps a
 * NaN a NaN through the bf16 narrowing; hm_round's bf16 carry can turn a NaN into an infinity or a zero, which the conv
 * contracts allow ("non-finite values give unspecified values").  The two must not be merged.
 */
#ifndef IS_HALF_MFMA_H_
#define IS_HALF_MFMA_H_
#include <type_traits>

#include "is_launch.h"

#define HM_HALF_DTYPE(DT) static_assert((DT) == IS_HEAD_F16 || (DT) == IS_HEAD_BF16, "a half dtype")

typedef float hm_acc16 __attribute__((ext_vector_type(16)));  /* C/D of the 32x32x16 shapes */
typedef float hm_acc4 __attribute__((ext_vector_type(4)));    /* C/D of the 16x16x32 shapes */
typedef _Float16 hm_f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 hm_bf16x8 __attribute__((ext_vector_type(8)));

/* fp32 -> half, round to nearest even, as 16 bits (the rounding of is_conv_pack_weights) */
template <int DT> __device__ __forceinline__ uint16_t hm_round(float v) {
    HM_HALF_DTYPE(DT);
    if constexpr (DT == IS_HEAD_F16) return __builtin_bit_cast(uint16_t, (_Float16)v);
    const uint32_t u = __float_as_uint(v);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
/* half -> fp32, exact */
template <int DT> __device__ __forceinline__ float hm_widen(uint16_t u) {
    HM_HALF_DTYPE(DT);
    if constexpr (DT == IS_HEAD_F16) return (float)__builtin_bit_cast(_Float16, u);
    return __uint_as_float((uint32_t)u << 16);
}

/* v_mfma_f32_32x32x16_{f16,bf16} and v_mfma_f32_16x16x32_{f16,bf16}: the accumulator's type picks the shape */
template <int DT> __device__ __forceinline__ hm_acc16 hm_mfma(uint4 a, uint4 b, hm_acc16 c) {
    HM_HALF_DTYPE(DT);
    if constexpr (DT == IS_HEAD_F16)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(hm_f16x8, a), __builtin_bit_cast(hm_f16x8, b), c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(hm_bf16x8, a), __builtin_bit_cast(hm_bf16x8, b), c, 0, 0, 0);
}
template <int DT> __device__ __forceinline__ hm_acc4 hm_mfma(uint4 a, uint4 b, hm_acc4 c) {
    HM_HALF_DTYPE(DT);
    if constexpr (DT == IS_HEAD_F16)
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(hm_f16x8, a), __builtin_bit_cast(hm_f16x8, b), c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(hm_bf16x8, a), __builtin_bit_cast(hm_bf16x8, b), c, 0, 0, 0);
}

/* the 16-byte slot of k half `h` of pixel `p` in a [pixel][2 halves of 8 channels] LDS tile: the two slots of a pixel
 * are swapped where bit 3 of the pixel index is set, so that the 16 lanes of a ds_read_b128 group, which read 16
 * consecutive pixels, cover all 16 slots of a bank row */
__device__ __forceinline__ int hm_slot(int p, int h) { return 2 * p + (h ^ ((p >> 3) & 1)); }

/* the C/D map of the 32x32 shapes: register i of a lane of half-wave `half` is this row of the block (the lane's
 * r = lane & 31 is the column) */
__device__ __forceinline__ int hm_cd_row(int i, int half) { return (i & 3) + 8 * (i >> 2) + 4 * half; }

/* round(scale * widen(round(w))): a folded BatchNorm scale on a weight as the forward pass rounded it */
template <int DT> __device__ __forceinline__ uint16_t hm_scaled_weight(float scale, float w) {
    float product = scale * hm_widen<DT>(hm_round<DT>(w));
    /* the fp32 product as a value: without this the compiler multiplies with v_fma_mixlo_f16, which rounds the exact
     * product to the half once and differs from round_half(fp32 product) in the double-rounding cases */
    asm volatile("" : "+v"(product));
    return hm_round<DT>(product);
}

/* The launchers' dispatch: f(std::integral_constant<int, DT>) for the half dtype (false: it is neither), and the
 * same for a choice of two compile-time values.  A launch is written once, in a generic lambda; they nest.  A launcher
 * that has checked its dtype before (it returns hipErrorInvalidValue first) may ignore the result. */
template <class F> static inline bool hm_dispatch(int dtype, F&& f) {
    if (dtype == IS_HEAD_F16) f(std::integral_constant<int, IS_HEAD_F16>{});
    else if (dtype == IS_HEAD_BF16) f(std::integral_constant<int, IS_HEAD_BF16>{});
    else return false;
    return true;
}
template <auto A, auto B, class F> static inline void hm_either(bool first, F&& f) {
    if (first) f(std::integral_constant<decltype(A), A>{});
    else f(std::integral_constant<decltype(B), B>{});
}

#endif /* IS_HALF_MFMA_H_ */
