/*
 * is_cnn_up.h -- the reference's fixed `up` layer (DRNSeg.py:35-44: ConvTranspose2d(C, C, 16, stride=8, padding=4,
 * groups=C) with fill_up_weights) as the kernels apply it to f13's planes without ever storing an upsampled value:
 * is_k_cnn_labels.hip (f15) and is_k_nll_up.hip (f16).  Its 1-D weights, their products for a row of 8 pixels, the
 * four-tap chain that the contract fixes bit for bit, and the staging of a tile of cells in LDS.
 */
#ifndef IS_CNN_UP_H_
#define IS_CNN_UP_H_

#include <hip/hip_runtime.h>

/* the 1-D weights of output position r = (o + 4) % 8: the tap on cell (o + 4) / 8 - 1 and the one on (o + 4) / 8 */
__device__ __forceinline__ float cnn_w_low(int r) { return (float)(15 - 2 * r) / 16.0f; }
__device__ __forceinline__ float cnn_w_high(int r) { return (float)(2 * r + 1) / 16.0f; }

/* the weight products of the 8 pixels k of one image row, whose own 1-D weights are wyl and wyh: pixel k has the
 * position r = (k + phase) & 7 (phase 4: k counts from a cell's left edge; 0: from the middle of the cell left of
 * it) */
__device__ __forceinline__ void cnn_up_weights(float (&w)[8][4], float wyl, float wyh, int phase) {
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int rk = (k + phase) & 7;
        w[k][0] = wyl * cnn_w_low(rk);
        w[k][1] = wyl * cnn_w_high(rk);
        w[k][2] = wyh * cnn_w_low(rk);
        w[k][3] = wyh * cnn_w_high(rk);
    }
}

/* the upsampled value of one pixel from its four cells (upper left, upper right, lower left, lower right), in the
 * contract's order */
__device__ __forceinline__ float cnn_up_chain(const float (&w)[4], float v00, float v01, float v10, float v11) {
    float acc = fmaf(w[0], v00, 0.0f);
    acc = fmaf(w[1], v01, acc);
    acc = fmaf(w[2], v10, acc);
    return fmaf(w[3], v11, acc);
}

/* Stages ROWS x PITCH cells of each of a frame's first n_classes planes [rows8][cols8] in tile[n_classes][ROWS][PITCH],
 * from the cell (cy0, cx0) on, with all THREADS threads of the workgroup.  A cell outside the plane is staged as
 * +0.0f: the taps have finite weights, so a tap on such a cell leaves the chain's value as it is
 * (fmaf(w, 0, acc) == acc), which is the contract's "skipped" and never 0 * inf.  (The one difference, a -0.0f
 * accumulator that becomes +0.0f, compares equal and so cannot move an arg-min.) */
template <int ROWS, int PITCH, int THREADS>
__device__ __forceinline__ void cnn_up_stage(float* tile, const float* frame, int n_classes, int cy0, int cx0,
                                             int rows8, int cols8, int tid) {
    const int P = rows8 * cols8;
    for (int i = tid; i < n_classes * (ROWS * PITCH); i += THREADS) {
        const int cls = i / (ROWS * PITCH), rem = i - cls * (ROWS * PITCH);
        const int ry = rem / PITCH, rx = rem - ry * PITCH;
        const int cy = cy0 + ry, cx = cx0 + rx;
        float v = 0.0f;
        if (cy >= 0 && cy < rows8 && cx >= 0 && cx < cols8) v = frame[(size_t)cls * P + cy * cols8 + cx];
        tile[i] = v;
    }
}

#endif /* IS_CNN_UP_H_ */
