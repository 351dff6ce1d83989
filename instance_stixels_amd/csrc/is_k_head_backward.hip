/*
 * is_k_head_backward.hip -- f14: the backward pass of the segmentation head (is_segmentation_head_backward).  The
 * contract is the header's section f14; the section's loss, is_semantic_nll, is is_k_nll.hip.
 *
 * k_head_backward_dx.  A wave owns 32 consecutive pixels of a frame, a lane one of them (l & 31) and the channels
 *   c = 2 s + (l >> 5), s = 0 .. 15: exactly the B operand of v_mfma_f32_32x32x2_f32 (lane l holds B[l >> 5][l & 31])
 *   for the contraction step over the channels (2 s, 2 s + 1), so dz never changes lanes.  Both half-waves read the
 *   class planes of gy for S, which is summed in increasing c in every lane.  dX: M = 32 features of a k-tile (the A
 *   operand: lane l holds w[2 s + (l >> 5)][k0 + (l & 31)], from an LDS image [channel][HB_KC features] whose channel
 *   stride puts the two half-waves on different banks), N = the 32 pixels, 16 steps in c order onto one accumulator:
 *   the contract's chain, the zero-padded channels leaving it as it is.  Accumulator register r of a half-wave is 128
 *   contiguous bytes of the dX plane of feature k0 + hb_row(r, half).
 * k_head_backward_partials.  One workgroup per (frame, chunk of IS_HEAD_BACKWARD_CHUNK pixels); its four waves work
 *   alone (no workgroup barrier), wave w on the k-tiles w, w + 4, ... one after the other, each over the whole chunk,
 *   so that a wave walks 32 feature rows contiguously and holds one accumulator.  M = the channels (A: lane l holds
 *   dz[l & 31][p + (l >> 5)]), N = the 32 features of a k-tile (B: lane l holds x[k0 + (l & 31)][p + (l >> 5)]), the
 *   contraction runs over the chunk's pixels in increasing p, 32 at a time.  Both operands are contiguous in p and a
 *   plane apart across the lanes, so a tile [32 rows][32 p] is loaded row by row (128 contiguous bytes per
 *   half-wave), kept in registers while the previous tiles are multiplied (the features two tiles ahead, dz, which
 *   comes from L2, one), written to the wave's LDS with the row stride 33 and read back transposed, conflict-free.
 *   Behind the end of the chunk dz is zero, which leaves an fmaf chain as it is.  db is the plain fp32 add chain of
 *   wave 0.
 * k_head_backward_reduce.  One thread per (c, k) and per c adds the partials in binary64, frame by frame, chunk by
 *   chunk.
 */
#include "is_launch.h"

#define HB_KC 128                        /* features per LDS weight image of k_head_backward_dx */
#define HB_WSTRIDE 160                   /* floats per channel of it: 32 mod 64, the half-waves on different banks */
#define HB_TSTRIDE 33                    /* floats per row of a [32][32] operand tile */
#define HB_TILE (32 * HB_TSTRIDE)
static_assert(IS_HEAD_MAX_CHANNELS == 32, "channels are one side of a 32x32 tile");
static_assert(IS_HEAD_BACKWARD_CHUNK % 64 == 0, "a chunk is whole tiles");

typedef float hb_acc __attribute__((ext_vector_type(16)));

template <int DT> struct HbFeature;
template <> struct HbFeature<IS_HEAD_F32> {
    typedef float type;
    static __device__ __forceinline__ float widen(float v) { return v; }
    static __device__ __forceinline__ float narrow(float v) { return v; }
};
template <> struct HbFeature<IS_HEAD_F16> {
    typedef _Float16 type;
    static __device__ __forceinline__ float widen(_Float16 v) { return (float)v; }
    static __device__ __forceinline__ _Float16 narrow(float v) { return (_Float16)v; } /* round to nearest even */
};
template <> struct HbFeature<IS_HEAD_BF16> {
    typedef uint16_t type;
    static __device__ __forceinline__ float widen(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }
    static __device__ __forceinline__ uint16_t narrow(float v) {
        const uint32_t u = __float_as_uint(v);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u); /* a NaN stays one */
        return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);                  /* round to nearest even */
    }
};

/* row of accumulator register `reg` in the half-wave `half` (the C/D map of the 32x32 MFMA shapes, as in f13) */
__device__ __forceinline__ int hb_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

template <int DT>
__global__ __launch_bounds__(256) void k_head_backward_dx(const float* __restrict__ y, const float* __restrict__ gy,
                                                          long long gy_stride, const float* __restrict__ weight,
                                                          float* __restrict__ dz_out, void* __restrict__ dx_, int K, int P,
                                                          int n_classes, int CH) {
    typedef typename HbFeature<DT>::type feat_t;
    __shared__ float wl[IS_HEAD_MAX_CHANNELS * HB_WSTRIDE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, half = lane >> 5;
    const int n = blockIdx.y;
    const int p = (blockIdx.x * 4 + wave) * 32 + j; /* a pixel outside the frame reads the last one and stores nothing */
    const bool inside = p < P;
    const size_t plane = (size_t)P;
    const float* yn = y + (size_t)n * CH * plane + min(p, P - 1);
    const float* gn = gy + (size_t)n * (size_t)gy_stride + min(p, P - 1);

    /* S in increasing c, in every lane; the loads first, all in flight at once */
    float g[IS_HEAD_MAX_CHANNELS];
#pragma unroll
    for (int c = 0; c < IS_HEAD_MAX_CHANNELS; ++c) g[c] = gn[(size_t)min(c, n_classes - 1) * plane];
    float yv[16], gv[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const size_t at = (size_t)min(2 * s + half, CH - 1) * plane;
        yv[s] = yn[at];
        gv[s] = gn[at];
    }
    double S = 0.0;
#pragma unroll
    for (int c = 0; c < IS_HEAD_MAX_CHANNELS; ++c)
        if (c < n_classes) S += (double)g[c];

    float dz[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const int c = 2 * s + half;
        float v = c < CH ? gv[s] : 0.0f;
        if (2 * s < n_classes) { /* wave-uniform: no exp for a step without a class */
            const float cls = (float)(exp(-(double)yv[s]) * S - (double)gv[s]);
            if (c < n_classes) v = cls;
        }
        dz[s] = v;
        if (inside && c < CH && dz_out) dz_out[((size_t)n * CH + c) * plane + p] = v;
    }
    if (!dx_) return;

    feat_t* dx = (feat_t*)dx_ + (size_t)n * K * plane + min(p, P - 1);
    for (int kc = 0; kc < K; kc += HB_KC) {
        __syncthreads(); /* the previous image is no longer read */
        for (int idx = tid; idx < IS_HEAD_MAX_CHANNELS * HB_KC; idx += 256) {
            const int c = idx / HB_KC, k = idx % HB_KC;
            const float v = weight[(size_t)min(c, CH - 1) * K + min(kc + k, K - 1)];
            wl[c * HB_WSTRIDE + k] = (c < CH && kc + k < K) ? v : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int kt = 0; kt < HB_KC / 32; ++kt) {
            const int k0 = kc + 32 * kt;
            if (k0 < K) {
                hb_acc acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
                for (int s = 0; s < 16; ++s)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wl[(2 * s + half) * HB_WSTRIDE + 32 * kt + j], dz[s], acc, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int k = k0 + hb_row(r, half);
                    if (inside && k < K) dx[(size_t)k * plane] = HbFeature<DT>::narrow(acc[r]);
                }
            }
        }
    }
}

template <int DT>
__global__ __launch_bounds__(256, 2) void k_head_backward_partials(const void* __restrict__ features_,
                                                                const float* __restrict__ dz, float* __restrict__ part,
                                                                int K, int P, int CH) {
    typedef typename HbFeature<DT>::type feat_t;
    __shared__ float lds[4][2][HB_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, half = lane >> 5;
    const int chunk = blockIdx.x, n = blockIdx.y, chunks = gridDim.x;
    const int pbeg = chunk * IS_HEAD_BACKWARD_CHUNK, pend = min(P, pbeg + IS_HEAD_BACKWARD_CHUNK);
    const size_t plane = (size_t)P;
    const float* dzn = dz + (size_t)n * CH * plane;
    const feat_t* xn = (const feat_t*)features_ + (size_t)n * K * plane;
    float* out = part + ((size_t)n * chunks + chunk) * CH * (size_t)(K + 1);
    float* dzt = lds[wave][0];
    float* xt = lds[wave][1];
    const int ktiles = (K + 31) / 32;

    /* Rows 2 i + half of a tile, pixel pt + j.  An address is a row base that is the same in every lane plus a 32-bit
     * byte offset of the lane (half a plane pair and the pixel: below 2^31 with P <= 2^28), which keeps the addresses
     * out of the vector registers; every address is clamped into the arrays.  dz is zero behind the chunk's end, which
     * leaves every chain as it is whatever finite feature stands beside it, so the features are not masked.  Rows
     * behind CH and K are not masked either: they only reach accumulator rows and columns that are never stored.
     * (K is even, so both rows of a pair are inside K or both are not; with an odd CH the last pair's upper row reads
     * the lower one.)  The mask is applied to the bits and hidden from the compiler, which turns a select on a loaded
     * value into a branch around the load with a full wait behind it. */
    auto load_dz = [&](float (&r)[16], int pt) {
        const int q = pt + j;
        const uint32_t low = (uint32_t)min(q, P - 1) * 4u, full = low + (uint32_t)half * (uint32_t)P * 4u;
        uint32_t keep = q < pend ? ~0u : 0u;
        asm volatile("" : "+v"(keep));
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const char* row = (const char*)(dzn + (size_t)(2 * i < CH ? 2 * i : 0) * plane);
            r[i] = __uint_as_float(__float_as_uint(*(const float*)(row + (2 * i + 1 < CH ? full : low))) & keep);
        }
    };
    auto load_x = [&](float (&r)[16], int kt, int pt) {
        const uint32_t at = ((uint32_t)min(pt + j, P - 1) + (uint32_t)half * (uint32_t)P) * (uint32_t)sizeof(feat_t);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int k2 = 32 * kt + 2 * i;
            r[i] = HbFeature<DT>::widen(*(const feat_t*)((const char*)(xn + (size_t)(k2 < K ? k2 : 0) * plane) + at));
        }
    };
    auto to_lds = [&](float* tile, const float (&r)[16]) {
#pragma unroll
        for (int i = 0; i < 16; ++i) tile[(2 * i + half) * HB_TSTRIDE + j] = r[i];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); /* read by the wave's other lanes; LDS serves a wave in order */
    };

    /* A wave takes the k-tiles wave, wave + 4, ... one after the other, each over the whole chunk: 32 feature rows are
     * walked contiguously, one accumulator is live.  (No workgroup barrier: the waves' trip counts differ.) */
    for (int kt = wave; kt < ktiles; kt += 4) {
        const bool with_bias = kt == 0;
        hb_acc acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        float bacc = 0.0f;
        /* dz one tile ahead (it comes from L2), the features two tiles ahead in two register sets with fixed roles */
        float dzr[16], xr0[16], xr1[16];
        auto step = [&](int pt, float (&xr)[16]) {
            to_lds(dzt, dzr);
            to_lds(xt, xr);
            load_dz(dzr, min(pt + 32, pend - 1)); /* behind the last tile: loaded in bounds and not used */
            load_x(xr, kt, min(pt + 64, pend - 1));
            __builtin_amdgcn_sched_barrier(0);
            if (with_bias) {
#pragma unroll 8
                for (int q = 0; q < 32; ++q) bacc = bacc + dzt[j * HB_TSTRIDE + q];
            }
#pragma unroll
            for (int s = 0; s < 16; ++s)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(dzt[j * HB_TSTRIDE + 2 * s + half],
                                                           xt[j * HB_TSTRIDE + 2 * s + half], acc, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        };
        load_dz(dzr, pbeg);
        load_x(xr0, kt, pbeg);
        load_x(xr1, kt, min(pbeg + 32, pend - 1));
        for (int pt = pbeg; pt < pend; pt += 64) {
            step(pt, xr0);
            if (pt + 32 < pend) step(pt + 32, xr1);
        }
        const int k = 32 * kt + j;
        if (k < K) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = hb_row(r, half);
                if (c < CH) out[(size_t)c * (K + 1) + k] = acc[r];
            }
        }
        if (with_bias && lane < CH) out[(size_t)lane * (K + 1) + K] = bacc;
    }
}

__global__ __launch_bounds__(256) void k_head_backward_reduce(const float* __restrict__ part, int n_parts, int K, int CH,
                                                              float* __restrict__ dw, float* __restrict__ db) {
    const int idx = blockIdx.x * 256 + threadIdx.x, total = CH * (K + 1);
    if (idx >= total) return;
    double s = 0.0;
#pragma unroll 8
    for (int w = 0; w < n_parts; ++w) s += (double)part[(size_t)w * total + idx];
    const int c = idx / (K + 1), k = idx % (K + 1);
    if (k < K) {
        if (dw) dw[(size_t)c * K + k] = (float)s;
    } else if (db) {
        db[c] = (float)s;
    }
}

static size_t hb_dz_bytes(int n_images, int Hs, int Ws, int channels) {
    const size_t bytes = (size_t)n_images * channels * Hs * Ws * sizeof(float);
    return (bytes + 15) & ~(size_t)15;
}
static int hb_chunks(int Hs, int Ws) { return (int)(((long long)Hs * Ws + IS_HEAD_BACKWARD_CHUNK - 1) / IS_HEAD_BACKWARD_CHUNK); }

/* dz of the batch (used when d_grad_logits is not given), then the chunk partials [n][chunks][CH][K + 1] */
extern "C" size_t isk_head_backward_scratch_bytes(int n_images, int K, int Hs, int Ws, int channels) {
    return hb_dz_bytes(n_images, Hs, Ws, channels) +
           (size_t)n_images * hb_chunks(Hs, Ws) * channels * (size_t)(K + 1) * sizeof(float);
}

/* The two instantiations for a feature type (IS_HEAD_*); null for any other value */
struct HeadBackwardKernels {
    decltype(&k_head_backward_dx<IS_HEAD_F32>) dx;
    decltype(&k_head_backward_partials<IS_HEAD_F32>) partials;
};
template <int DT>
static HeadBackwardKernels head_backward_kernels_of() { return {k_head_backward_dx<DT>, k_head_backward_partials<DT>}; }
static HeadBackwardKernels head_backward_kernels(int dtype) {
    switch (dtype) {
    case IS_HEAD_F32: return head_backward_kernels_of<IS_HEAD_F32>();
    case IS_HEAD_F16: return head_backward_kernels_of<IS_HEAD_F16>();
    case IS_HEAD_BF16: return head_backward_kernels_of<IS_HEAD_BF16>();
    }
    return {nullptr, nullptr};
}

/* The arguments are checked by is_segmentation_head_backward. */
extern "C" hipError_t isk_launch_segmentation_head_backward(const is_segmentation_head_backward_args* a, hipStream_t stream) {
    const int CH = a->n_classes + a->n_regression, P = a->rows8 * a->cols8, chunks = hb_chunks(a->rows8, a->cols8);
    const bool contract = a->d_grad_weight || a->d_grad_bias;
    float* scratch_dz = (float*)a->d_scratch;
    float* part = (float*)((char*)a->d_scratch + hb_dz_bytes(a->n_images, a->rows8, a->cols8, CH));
    /* the contraction reads dz from d_grad_logits where that is given, from the scratch otherwise */
    float* dz_a = a->d_grad_logits ? a->d_grad_logits : contract ? scratch_dz : nullptr;
    const dim3 grid_a((P + 127) / 128, a->n_images), grid_b(chunks, a->n_images);
    const HeadBackwardKernels k = head_backward_kernels(a->dtype);
    if (k.dx == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k.dx, grid_a, dim3(256), 0, stream, a->d_cnn_out, a->d_grad_out, a->grad_image_stride, a->d_weight, dz_a,
                       a->d_grad_features, a->K, P, a->n_classes, CH);
    if (contract)
        hipLaunchKernelGGL(k.partials, grid_b, dim3(256), 0, stream, a->d_features, (const float*)dz_a, part, a->K, P, CH);
    if (contract)
        hipLaunchKernelGGL(k_head_backward_reduce, dim3((CH * (a->K + 1) + 255) / 256), dim3(256), 0, stream,
                           (const float*)part, a->n_images * chunks, a->K, CH, a->d_grad_weight, a->d_grad_bias);
    return hipGetLastError();
}
