/*
 * is_k_conv_backward.hip -- f21, and f22's launcher: the backward pass of is_conv_bn at stride 1 (a 3x3 dilated or 1x1 convolution, folded
 * BatchNorm frozen at its running statistics, optional residual, optional ReLU): the masked gradient gh, dshift, the
 * transposed pack for dX, the weight-gradient partials G, their reduction to dW, and dscale.  dX itself is
 * is_k_conv3x3.hip's launch (isk_launch_conv_bn) on gh and the transposed pack; that file is not touched.
 *
 * Numerics contract: include/instance_stixels_core.h f21, DESIGN.md 10aa.  In short: gh is the half rounding of dY under the
 * ReLU mask of the STORED output; everything else is computed from gh.  dshift, Gsum, dW and dscale are binary64 sums in
 * an order the shape fixes; G's chunk partials are fp32 MFMA accumulators, one per (co, ci, tap) and chunk, fed in an
 * order the shape fixes.  No floating-point atomics; the same bytes on every run and for every choice of outputs.
 *
 * k_conv_bwd_weight<DT, TAPS>, the hot kernel, is the implicit GEMM that is_conv_backward.h describes and holds (tile
 * mapping, staging, LDS tile and bank account, loads one step ahead), here at STEP = 1: the x operand of tap (ky, kx) is
 * x[ci][y + (ky - 1) d][p + (kx - 1) d].  What this file adds is the row schedule: the rows of a segment go by in residue
 * classes mod d (y = ya + res, ya + res + d, ...), so that the rows y - d, y, y + d of a step are the previous, this and
 * the next row of the class in the ring.  A step stages gh and the one new row in its three kx copies: 4 tiles (10 at
 * the first step of a class) for 18 MFMAs per wave, where staging every tap's tile took 10.
 */
#include "is_conv_backward.h"

#define CB_PREP_ITEMS 8            /* elements of a thread of k_conv_bwd_prepare */
#define CB_PREP_BLOCK (256 * CB_PREP_ITEMS)

/* The sum of the 256 threads' values in binary64: t += t + s for s = 128 .. 1.  `lds` holds 256 doubles; every thread
 * of the block calls, and gets the sum. */
__device__ __forceinline__ double cb_block_sum(double v, double* lds) {
    const int tid = threadIdx.x;
    __syncthreads(); /* (the previous use of lds is over) */
    lds[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) lds[tid] = lds[tid] + lds[tid + s];
        __syncthreads();
    }
    return lds[0];
}

/* gh and the dshift block sums.  Grid (blocks of a plane, co, n); a thread takes 8 consecutive elements of the plane.
 * vec: P % 8 == 0 and every base and stride keeps a thread's 8 elements 16-byte aligned (32 for an fp32 operand). */
template <int DT>
__global__ __launch_bounds__(256) void k_conv_bwd_prepare(const void* __restrict__ out_, int out_f32, int relu,
                                                          const void* __restrict__ dy_, int dy_f32, long long dy_stride,
                                                          uint16_t* __restrict__ gh, double* __restrict__ shift_part,
                                                          int Cout, int P, int vec) {
    __shared__ double lds[256];
    const int tid = threadIdx.x, co = blockIdx.y, n = blockIdx.z;
    const int e0 = blockIdx.x * CB_PREP_BLOCK + tid * CB_PREP_ITEMS;
    const size_t plane = ((size_t)n * Cout + co) * P;
    const size_t dplane = (size_t)n * (size_t)dy_stride + (size_t)co * P;
    float g[CB_PREP_ITEMS];
    uint16_t keep[CB_PREP_ITEMS];
    if (vec && e0 >= P) { /* (past the plane: +0 into the block's sum, nothing stored) */
#pragma unroll
        for (int j = 0; j < 8; ++j) g[j] = 0.0f, keep[j] = 0u;
    } else if (vec) { /* (P % 8 == 0: the 8 elements are inside together) */
        if (dy_f32) {
            const float4 a = *(const float4*)((const float*)dy_ + dplane + e0), b = *(const float4*)((const float*)dy_ + dplane + e0 + 4);
            g[0] = a.x, g[1] = a.y, g[2] = a.z, g[3] = a.w, g[4] = b.x, g[5] = b.y, g[6] = b.z, g[7] = b.w;
        } else {
            const uint4 q = *(const uint4*)((const uint16_t*)dy_ + dplane + e0);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) g[j] = hm_widen<DT>((uint16_t)(w[j >> 1] >> (16 * (j & 1))));
        }
        if (!relu) {
#pragma unroll
            for (int j = 0; j < 8; ++j) keep[j] = 0xffffu;
        } else if (out_f32) {
            const float4 a = *(const float4*)((const float*)out_ + plane + e0), b = *(const float4*)((const float*)out_ + plane + e0 + 4);
            const float o[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) keep[j] = o[j] > 0.0f ? 0xffffu : 0u;
        } else {
            const uint4 q = *(const uint4*)((const uint16_t*)out_ + plane + e0);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) keep[j] = hm_widen<DT>((uint16_t)(w[j >> 1] >> (16 * (j & 1)))) > 0.0f ? 0xffffu : 0u;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int e = min(e0 + j, P - 1); /* (past the plane: loaded in bounds, masked below) */
            g[j] = dy_f32 ? ((const float*)dy_)[dplane + e] : hm_widen<DT>(((const uint16_t*)dy_)[dplane + e]);
            float o = 1.0f;
            if (relu) o = out_f32 ? ((const float*)out_)[plane + e] : hm_widen<DT>(((const uint16_t*)out_)[plane + e]);
            keep[j] = (e0 + j < P && o > 0.0f) ? 0xffffu : 0u;
        }
    }
    uint16_t h[CB_PREP_ITEMS];
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        h[j] = hm_round<DT>(g[j]) & keep[j];
        s = s + (double)hm_widen<DT>(h[j]);
    }
    if (vec) {
        if (e0 < P) {
            uint4 q;
            q.x = h[0] | ((uint32_t)h[1] << 16), q.y = h[2] | ((uint32_t)h[3] << 16);
            q.z = h[4] | ((uint32_t)h[5] << 16), q.w = h[6] | ((uint32_t)h[7] << 16);
            *(uint4*)(gh + plane + e0) = q;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (e0 + j < P) gh[plane + e0 + j] = h[j];
    }
    if (shift_part) { /* (the same for the whole grid) */
        const double total = cb_block_sum(s, lds);
        if (tid == 0) shift_part[((size_t)n * Cout + co) * gridDim.x + blockIdx.x] = total;
    }
}

/* The transposed, tap-flipped, scaled pack in is_conv_pack_weights' layout for (channels_out' = Cin, channels_in' = Cout):
 * packed[((tile * chunks + chunk) * taps + t) * 512 + h * 256 + r * 8 + j] = round(scale[co] * w_half[co][ci][taps - 1 - t])
 * with ci = 32 tile + r, co = 16 chunk + 8 h + j; and the launch's scale 1 and shift 0, [Cin] each. */
template <int DT>
__global__ __launch_bounds__(256) void k_conv_bwd_pack_t(const float* __restrict__ weight, const float* __restrict__ scale,
                                                         uint16_t* __restrict__ packed, float* __restrict__ ones,
                                                         float* __restrict__ zeros, int Cin, int Cout, int taps, int total) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < Cin) ones[e] = 1.0f, zeros[e] = 0.0f;
    if (e >= total) return;
    const int j = e & 7, r = (e >> 3) & 31, h = (e >> 8) & 1, t = (e >> 9) % taps, blk = (e >> 9) / taps;
    const int chunks = Cout / 16, chunk = blk % chunks, tile = blk / chunks;
    const int ci = 32 * tile + r, co = 16 * chunk + 8 * h + j;
    packed[e] = hm_scaled_weight<DT>(scale[co], weight[((size_t)co * Cin + ci) * taps + (taps - 1 - t)]);
}

/* part[((chunk * TAPS + tap) * Cout + co) * Cin + ci], chunk = image * bands + band */
template <int DT, int TAPS>
__global__ __launch_bounds__(256) void k_conv_bwd_weight(const uint16_t* __restrict__ gh, const uint16_t* __restrict__ x,
                                                         float* __restrict__ part, int Cin, int Cout, int H, int W, int d_,
                                                         int bands, int tiles_ci, int tiles, int chunks) {
    static_assert(TAPS == 9 || TAPS == 1, "a 3x3 or a 1x1 convolution");
    const int d = TAPS == 1 ? 0 : d_;
    constexpr int KX = TAPS == 9 ? 3 : 1;
    const cb_group g = cb_decode<IS_CONV_BACKWARD_BAND>(H, bands, tiles_ci, tiles);
    if (g.chunk >= chunks) return; /* (the whole workgroup, before any barrier) */
    const int ya = g.ya, yb = g.yb, co0 = g.co0, ci0 = g.ci0;
    const cb_planes ghn = cb_image(gh, g.n, co0, Cout, H, W), xn = cb_image(x, g.n, ci0, Cin, H, W);
    hm_acc16 acc[TAPS];
    cb_clear(acc);

    /* 3x3: for a segment, the rows of the chunk go by in residue classes mod d: y = ya + res, ya + res + d, ...; step t
     * of a class needs the x rows t - 1, t, t + 1 of that class (image rows y - d, y, y + d), which stay in a ring of
     * three rows per kx copy: row j of the class lives in ring slot (j + 1) % 3.  The first step of a class stages rows
     * -1, 0 and 1, every later step row t + 1 alone, over the slot of row t - 2: 3 staged x tiles and gh per step. */
    const int classes = TAPS == 1 ? 1 : min(d, yb - ya), stride = TAPS == 1 ? 1 : d;
    auto load_b = [&](int gy, uint32_t (&v)[4][KX][2], int xs) { cb_load_b<KX, 1>(v, xn, gy, xs, d); };
    auto store_b = [&](int slot, int gy, const uint32_t (&v)[4][KX][2], int xs) { cb_store_b<KX, 1>(slot, v, xn, gy, xs, d); };

    uint32_t va[4][2], vb[4][KX][2];
    for (int xs = 0; xs < W; xs += CB_SEG) {
        for (int res = 0; res < classes; ++res) {
            const int y0 = ya + res; /* row j of the class is image row y0 + j d */
            __syncthreads(); /* the previous class's operands are no longer read */
            if (TAPS == 9) { /* rows -1 and 0 of the class, staged as they come; row 1 goes the common way */
                load_b(y0 - d, vb, xs), store_b(0, y0 - d, vb, xs);
                load_b(y0, vb, xs), store_b(1, y0, vb, xs);
            }
            cb_load_a(va, ghn, y0, xs);
            load_b(TAPS == 9 ? y0 + d : y0, vb, xs);
            int t = 0;
            for (int y = y0; y < yb; y += stride, ++t) {
                if (t > 0) __syncthreads(); /* the previous step's operands are no longer read */
                cb_store_a(va, ghn, xs);
                store_b(TAPS == 9 ? (t + 2) % 3 : 0, TAPS == 9 ? y + d : y, vb, xs);
                __syncthreads();
                if (y + stride < yb) { /* the next step's operands, in flight while this step multiplies */
                    cb_load_a(va, ghn, y + stride, xs);
                    load_b(TAPS == 9 ? y + 2 * d : y + stride, vb, xs);
                }
                CB_MULTIPLY(DT, TAPS, acc, g, t % 3); /* tap (ky, kx): row t + ky - 1 of the class, copy kx */
            }
        }
    }
    cb_store_part<TAPS>(part, acc, g, Cout, Cin);
}

/* One thread per (tap, co, ci) of the partials' layout: Gsum in binary64 over the chunks in increasing order (image
 * outer, band inner), dW and Gsum in conv.weight's layout. */
__global__ __launch_bounds__(256) void k_conv_bwd_reduce(const float* __restrict__ part, int chunks, int Cin, int Cout,
                                                         int taps, const float* __restrict__ scale, float* __restrict__ dw,
                                                         double* __restrict__ gsum) {
    const int total = taps * Cout * Cin, idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    double s = 0.0;
#pragma unroll 8
    for (int c = 0; c < chunks; ++c) s = s + (double)part[(size_t)c * total + idx];
    const int ci = idx % Cin, co = (idx / Cin) % Cout, tap = idx / (Cin * Cout);
    const size_t at = ((size_t)co * Cin + ci) * taps + tap;
    if (dw) dw[at] = (float)((double)scale[co] * s);
    if (gsum) gsum[at] = s;
}

/* One block per co: dscale from Gsum and w_half, dshift from the block sums of k_conv_bwd_prepare; each a sum of
 * contiguous thread ranges in increasing index, then the LDS tree. */
template <int DT>
__global__ __launch_bounds__(256) void k_conv_bwd_channel(const double* __restrict__ gsum, const float* __restrict__ weight,
                                                          const double* __restrict__ shift_part, int n_images, int pblocks,
                                                          int Cin, int Cout, int taps, float* __restrict__ dscale,
                                                          float* __restrict__ dshift) {
    __shared__ double lds[256];
    const int tid = threadIdx.x, co = blockIdx.x;
    if (dscale) {
        const int items = Cin * taps, per = (items + 255) / 256;
        const size_t base = (size_t)co * items;
        double s = 0.0;
        for (int i = tid * per; i < min((tid + 1) * per, items); ++i)
            s = s + (double)hm_widen<DT>(hm_round<DT>(weight[base + i])) * gsum[base + i];
        const double total = cb_block_sum(s, lds);
        if (tid == 0) dscale[co] = (float)total;
    }
    if (dshift) {
        const long long items = (long long)n_images * pblocks, per = (items + 255) / 256;
        double s = 0.0;
        for (long long i = tid * per; i < min((tid + 1) * per, items); ++i) {
            const long long img = i / pblocks, blk = i % pblocks;
            s = s + shift_part[((size_t)img * Cout + co) * pblocks + blk];
        }
        const double total = cb_block_sum(s, lds);
        if (tid == 0) dshift[co] = (float)total;
    }
}

static int cb_pblocks(int H, int W) { return (int)(((long long)H * W + CB_PREP_BLOCK - 1) / CB_PREP_BLOCK); }

/* the sections of the scratch, in this order, each 16-byte aligned */
struct cb_scratch {
    size_t gh, packed, ones, zeros, shift_part, gsum, part, end;
};
/* H, W: the OUTPUT's extents (the input's at stride 1) */
static cb_scratch cb_layout(int n, int Cin, int Cout, int H, int W, int kernel, int stride) {
    const size_t taps = (size_t)kernel * kernel, P = (size_t)H * W;
    cb_scratch s;
    s.gh = 0;
    s.packed = s.gh + cb_align16((size_t)n * Cout * P * 2);
    s.ones = s.packed + cb_align16((size_t)Cin * Cout * taps * 2);
    s.zeros = s.ones + cb_align16((size_t)Cin * 4);
    s.shift_part = s.zeros + cb_align16((size_t)Cin * 4);
    s.gsum = s.shift_part + cb_align16((size_t)n * Cout * cb_pblocks(H, W) * 8);
    s.part = s.gsum + cb_align16((size_t)Cout * Cin * taps * 8);
    s.end = s.part + cb_align16((size_t)n * cb_bands(H, stride) * taps * Cout * Cin * 4);
    return s;
}

extern "C" size_t isk_conv_backward_scratch_bytes(int n_images, int channels_in, int channels_out, int rows_in, int cols_in,
                                                  int kernel, int stride) {
    const int H = (rows_in + stride - 1) / stride, W = (cols_in + stride - 1) / stride;
    if (!cb_weight_grid(n_images, channels_in, channels_out, cb_bands(H, stride))) return 0;
    return cb_layout(n_images, channels_in, channels_out, H, W, kernel, stride).end;
}

/* The arguments are checked by is_core.hip's conv_bn_backward_run, for is_conv_bn_backward and
 * is_conv_bn_stride_backward alike.  H, W: the OUTPUT's extents, which gh, dshift and the chunks go by. */
extern "C" hipError_t isk_launch_conv_bn_backward(const is_conv_bn_stride_backward_args* a, hipStream_t stream) {
    const int n = a->n_images, Cin = a->channels_in, Cout = a->channels_out, s2 = a->stride == 2;
    const int H = (a->rows_in + a->stride - 1) / a->stride, W = (a->cols_in + a->stride - 1) / a->stride;
    const int taps = a->kernel * a->kernel, P = H * W, pblocks = cb_pblocks(H, W), bands = cb_bands(H, a->stride), chunks = n * bands;
    const cb_scratch lay = cb_layout(n, Cin, Cout, H, W, a->kernel, a->stride);
    char* const scratch = (char*)a->d_scratch;
    uint16_t* const gh = a->d_grad_pre ? (uint16_t*)a->d_grad_pre : (uint16_t*)(scratch + lay.gh);
    uint16_t* const packed = (uint16_t*)(scratch + lay.packed);
    float* const ones = (float*)(scratch + lay.ones);
    float* const zeros = (float*)(scratch + lay.zeros);
    double* const shift_part = (double*)(scratch + lay.shift_part);
    double* const gsum = (double*)(scratch + lay.gsum);
    float* const part = (float*)(scratch + lay.part);
    const bool contract = a->d_grad_weight || a->d_grad_scale;
    if (a->dtype != IS_HEAD_F16 && a->dtype != IS_HEAD_BF16) return hipErrorInvalidValue;
    if (a->kernel != 3 && a->kernel != 1) return hipErrorInvalidValue;

    {   /* gh, and the dshift block sums where dshift is asked for */
        const int out_f32 = a->out_dtype == IS_HEAD_F32, dy_f32 = a->grad_out_dtype == IS_HEAD_F32;
        /* a thread's 8 elements are one 16-byte access of a half operand, two of an fp32 one */
        const bool aligned = (uintptr_t)gh % 16 == 0 && (uintptr_t)a->d_grad_out % (dy_f32 ? 32 : 16) == 0 &&
                             (!a->relu || (uintptr_t)a->d_out % (out_f32 ? 32 : 16) == 0);
        const int vec = P % 8 == 0 && a->grad_image_stride % 8 == 0 && aligned;
        const dim3 grid(pblocks, Cout, n);
        double* const sp = a->d_grad_shift ? shift_part : nullptr;
        hm_dispatch(a->dtype, [&](auto dt) {
            hipLaunchKernelGGL(k_conv_bwd_prepare<dt()>, grid, dim3(256), 0, stream, a->d_out, out_f32, a->relu,
                               a->d_grad_out, dy_f32, a->grad_image_stride, gh, sp, Cout, P, vec);
        });
    }
    if (a->d_grad_features) { /* the transposed pack, then (stride 1) f18's launch with the channels swapped */
        const int total = Cin * Cout * taps;
        const dim3 grid((total + 255) / 256);
        hm_dispatch(a->dtype, [&](auto dt) {
            hipLaunchKernelGGL(k_conv_bwd_pack_t<dt()>, grid, dim3(256), 0, stream, a->d_weight, a->d_scale, packed, ones,
                               zeros, Cin, Cout, taps, total);
        });
        if (s2) { /* the gather form of the transposed convolution (is_k_conv_backward_stride.hip) */
            isk_launch_conv_bwd_data_s2(a, gh, packed, stream);
        } else {
            is_conv_bn_stride_args c = {};
            c.d_features = gh, c.dtype = a->dtype, c.n_images = n, c.channels_in = Cout, c.channels_out = Cin;
            c.rows_in = H, c.cols_in = W, c.kernel = a->kernel, c.stride = 1, c.dilation = a->dilation;
            c.d_packed = packed, c.d_scale = ones, c.d_shift = zeros, c.d_residual = a->d_grad_features_add, c.relu = 0;
            c.d_out = a->d_grad_features, c.out_dtype = a->grad_features_dtype;
            const hipError_t e = isk_launch_conv_bn(&c, stream);
            if (e != hipSuccess) return e;
        }
    }
    if (contract && s2) isk_launch_conv_bwd_weight_s2(a, gh, part, stream);
    if (contract && !s2) {
        const int tiles_ci = (Cin + 63) / 64, tiles = tiles_ci * ((Cout + 63) / 64);
        const dim3 grid((unsigned)cb_weight_grid(n, Cin, Cout, bands));
        hm_dispatch(a->dtype, [&](auto dt) {
            hm_either<9, 1>(taps == 9, [&](auto t) {
                hipLaunchKernelGGL((k_conv_bwd_weight<dt(), t()>), grid, dim3(256), cb_weight_lds(taps), stream,
                                   (const uint16_t*)gh, (const uint16_t*)a->d_features, part, Cin, Cout, H, W, a->dilation,
                                   bands, tiles_ci, tiles, chunks);
            });
        });
    }
    if (contract) /* (taps * Cout * Cin is at most 9 * 2^22) */
        isk_launch_conv_bwd_reduce(part, chunks, Cin, Cout, taps, a->d_scale, a->d_grad_weight, a->d_grad_scale ? gsum : nullptr, stream);
    if (a->d_grad_scale || a->d_grad_shift)
        isk_launch_conv_bwd_channel(a->dtype, gsum, a->d_weight, shift_part, n, pblocks, Cin, Cout, taps, a->d_grad_scale,
                                    a->d_grad_shift, stream);
    return hipGetLastError();
}

/* The two reductions; f23 (is_k_stem_backward.hip) runs them on the stem's partials: the same kernels, the same
 * instantiations. */
extern "C" void isk_launch_conv_bwd_reduce(const float* part, int chunks, int Cin, int Cout, int taps, const float* scale,
                                           float* dw, double* gsum, hipStream_t stream) {
    const int total = taps * Cout * Cin;
    hipLaunchKernelGGL(k_conv_bwd_reduce, dim3((total + 255) / 256), dim3(256), 0, stream, part, chunks, Cin, Cout, taps,
                       scale, dw, gsum);
}

extern "C" void isk_launch_conv_bwd_channel(int dtype, const double* gsum, const float* weight, const double* shift_part,
                                            int n_images, int pblocks, int Cin, int Cout, int taps, float* dscale,
                                            float* dshift, hipStream_t stream) {
    /* (the callers have checked the dtype: is_core.hip's shape checks, isk_launch_stem_backward) */
    hm_dispatch(dtype, [&](auto dt) {
        hipLaunchKernelGGL(k_conv_bwd_channel<dt()>, dim3(Cout), dim3(256), 0, stream, gsum, weight, shift_part, n_images,
                           pblocks, Cin, Cout, taps, dscale, dshift);
    });
}
