/*
 * is_cnn_up.h -- the 1-D weights of the reference's fixed `up` layer (DRNSeg.py:35-44: ConvTranspose2d(C, C, 16,
 * stride=8, padding=4, groups=C) with fill_up_weights), shared by the kernels that apply it to f13's planes without
 * ever storing an upsampled value: is_k_cnn_labels.hip (f15) and is_k_nll_up.hip (f16).
 */
#ifndef IS_CNN_UP_H_
#define IS_CNN_UP_H_

#include <hip/hip_runtime.h>

/* the 1-D weights of output position r = (o + 4) % 8: the tap on cell (o + 4) / 8 - 1 and the one on (o + 4) / 8 */
__device__ __forceinline__ float cnn_w_low(int r) { return (float)(15 - 2 * r) / 16.0f; }
__device__ __forceinline__ float cnn_w_high(int r) { return (float)(2 * r + 1) / 16.0f; }

#endif /* IS_CNN_UP_H_ */
