/*
 * ref_shim.h -- force-included (`-include`) ahead of every hipified translation unit of the
 * upstream reference that `make -C oracle ref` compiles into oracle/_ref/libref_stixels.so.
 *
 * TEST INFRASTRUCTURE ONLY.  The reference text itself is not edited (hipify-perl's own rewrite
 * is the only change); everything that differs between the CUDA build and this gfx950 build is
 * one of the substitutions below, each with its reason.
 *
 *  1. __shfl(v, l)      -> __shfl(v, l, 32)
 *     __shfl_up(v, d)   -> __shfl_up(v, d, 32)
 *     The reference is written for 32-lane warps (util.h: WARP_SIZE = 32) and takes the
 *     pre-Volta branch `#if (__CUDA_ARCH__ < 700)` under hipcc (__CUDA_ARCH__ is undefined,
 *     so the test reads 0 < 700).  A gfx950 wave is 64 lanes wide and HIP's default width is
 *     warpSize: without an explicit width the scan of ComputeObjectLUT (one fn per 32-lane
 *     group) would pull lanes across the two halves of a wave, and warp_prefix_sum's final
 *     `__shfl(cost, WARP_SIZE-1)` would hand the upper half the lower half's carry.  Width 32
 *     makes each half-wave an independent 32-lane warp, which is the reference's model.
 *
 *  2. __logf(x)         -> is_logf(x)
 *     logf(x)           -> is_logf(x) in device code, libm logf(x) in host code
 *     The canonical numerics of this project (oracle/stixels_oracle.c header):
 *     CUDA's __logf is an approximate intrinsic with no bit-exact gfx950 equivalent, and the
 *     device logf of two vendor libraries need not agree bit for bit.  The project fixes both
 *     to is_logf (include/is_numerics.h, within 1 ulp of libm), which the HIP kernels and the
 *     CPU oracle use alike.  Host code (Stixels::Initialize / PrecomputeGround / ...) keeps
 *     libm, as the reference's host build does.
 *
 * The compile line adds -O2 -ffp-contract=off -fno-fast-math -DNDEBUG: IEEE fp32 without FMA
 * contraction (hipcc would contract by default), correctly rounded fp32 division and sqrt
 * (hipcc's default, stated on the command line), and the reference's device asserts compiled
 * out as in its release build -- the host checks of oracle/ref_driver.hip take their place.
 */
#ifndef REF_SHIM_H_
#define REF_SHIM_H_

#include <hip/hip_runtime.h>
#include <math.h>
#include "is_numerics.h"

static __host__ __device__ __forceinline__ float ref_shim_logf(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return is_logf(x);
#else
    return logf(x);
#endif
}

#define __shfl(v, l) __shfl((v), (l), 32)
#define __shfl_up(v, d) __shfl_up((v), (d), 32)
#define __logf(x) is_logf(x)
#define logf(x) ref_shim_logf(x)

#endif /* REF_SHIM_H_ */
