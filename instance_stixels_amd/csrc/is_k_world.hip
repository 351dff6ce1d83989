/* is_k_world.hip -- the 3-D stixel world of a batch (is_stixel_world of instance_stixels_core.h): one 96-byte
 * record per section in front of a column's terminator, in (image, column, section) order, with the section's
 * fields, its cluster label and the twelve floats of its four 3-D corners.  It is what the reference's live path
 * hands to its consumers per frame (Compute -> GetInstanceStixels -> Get3DVertices -> populateStixelsArray); here
 * for every frame of a batch in one launch sequence:
 *   k_count_sections / k_scan_counts   (is_k_pack.hip) counts and offsets of the columns, offsets[n] = the total
 *   k_world                            wave per column, lanes over its sections: a Section as two 16-byte loads,
 *                                      the records through LDS as contiguous 16-byte stores of the wave
 * The vertices are the expressions of Stixels::Get3DVertices in fp32 with its operand order (the build has no
 * contraction and an IEEE division), so a finite value has the host's bits; a zero disparity gives its +-inf, and
 * NaN where the host has NaN.  The road parameters of the frames travel as kernel arguments (IS_WORLD_IMAGES frames
 * per launch), so nothing is allocated or copied per call. */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "instance_stixels_core.h"
#include "is_launch.h"

static_assert(sizeof(is_world_stixel) == 96 && sizeof(is_section) == 32, "k_world moves 16-byte chunks");

#define IS_WORLD_IMAGES 64 /* frames per launch: their road parameters are 512 bytes of kernel arguments */

struct WorldRoad {
    float alpha_ground[IS_WORLD_IMAGES];
    int vhor[IS_WORLD_IMAGES];
};

struct WorldArgs {
    const is_section* sections;
    const int32_t* section_instance; /* may be null */
    const int32_t* counts;
    const int32_t* offsets;
    is_world_stixel* world;
    int32_t* frame_totals;
    int first_image, n_images; /* of this launch */
    int realcols, S, rows, column_step, capacity;
    float focal, baseline, cx, cy;
};

/* -z / focal * (center - p), Get3DVertices' expression for x and y */
__device__ __forceinline__ float world_xy(float z, float focal, float center, float p) {
    return -z / focal * (center - p);
}

/* One 16-byte chunk of a record.  The empty asm keeps the four words one value: without it the compiler takes the
 * six chunks apart and joins the words again across the chunk borders. */
typedef int v4i __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void put16(int4* dst, int x, int y, int z, int w) {
    v4i v = {x, y, z, w};
    asm volatile("" : "+v"(v));
    *reinterpret_cast<v4i*>(dst) = v;
}

/* Wave per column, 64 sections per round.  Every lane builds the record of its section in the wave's LDS slab
 * (64 x 96 B); the wave then writes the round's contiguous records x 96 bytes with consecutive lanes on consecutive
 * 16-byte chunks.  (Measured against each lane storing its own record, neighbouring lanes 96 B apart: 50 us
 * against 62 us for the three launches of 64 frames at 1024x2048) */
__global__ __launch_bounds__(256) void k_world(const WorldArgs a, const WorldRoad road) {
    __shared__ int4 s_rec[4 * 64 * 6];
    int4* const mine = s_rec + (threadIdx.x >> 6) * 64 * 6;
    const int local = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (local >= a.n_images * a.realcols) return;
    const int li = local / a.realcols, c = local - li * a.realcols; /* wave-uniform */
    const int col = a.first_image * a.realcols + local;
    const int n = a.counts[col], base = a.offsets[col];
    if (c == 0 && lane == 0) a.frame_totals[a.first_image + li] = a.offsets[col + a.realcols] - base;
    const float alpha = road.alpha_ground[li];
    const int vhor = road.vhor[li];
    const int4* src = reinterpret_cast<const int4*>(a.sections + (size_t)col * a.S);
    const int32_t* inst = a.section_instance ? a.section_instance + (size_t)col * a.S : nullptr;
    const float x_l = (float)(c * a.column_step), x_r = x_l + (float)a.column_step;
    const float bf = a.baseline * a.focal;
    const auto f = [](float v) { return __float_as_int(v); };
    for (int i0 = 0; i0 < n && base + i0 < a.capacity; i0 += 64) {
        const int m = min(min(n - i0, 64), a.capacity - (base + i0)); /* records of this round, >= 1 */
        const int i = i0 + lane;
        if (lane < m) {
            const int4 lo = src[2 * i], hi = src[2 * i + 1];
            const int id = inst ? inst[i] : -1;
            const int type = lo.x, vB = lo.y, vT = lo.z;
            const float y_t = (float)(a.rows - vT - 1), y_b = (float)(a.rows - vB);
            float top = 0.0f, bottom = 0.0f; /* sky stays at depth 0 */
            if (type == IS_OBJECT) {
                top = bf / __int_as_float(lo.w);
                bottom = top;
            } else if (type == IS_GROUND) {
                top = bf / (alpha * (float)(vhor - vT));
                bottom = bf / (alpha * (float)(vhor - vB));
            }
            const float tlx = world_xy(top, a.focal, a.cx, x_l), trx = world_xy(top, a.focal, a.cx, x_r);
            const float ty = world_xy(top, a.focal, a.cy, y_t);
            const float brx = world_xy(bottom, a.focal, a.cx, x_r), blx = world_xy(bottom, a.focal, a.cx, x_l);
            const float by = world_xy(bottom, a.focal, a.cy, y_b);
            int4* rec = mine + lane * 6;
            put16(rec + 0, c, i, type, vB);
            put16(rec + 1, vT, hi.x, id, lo.w);                 /* vT, class, id, disparity */
            put16(rec + 2, hi.y, hi.z, hi.w, f(tlx));           /* cost, mean x, mean y | TL.x */
            put16(rec + 3, f(ty), f(top), f(trx), f(ty));       /* TL.y TL.z | TR.x TR.y */
            put16(rec + 4, f(top), f(brx), f(by), f(bottom));   /* TR.z | BR */
            put16(rec + 5, f(blx), f(by), f(bottom), 0);        /* BL | reserved */
        }
        /* (one wave: its LDS operations complete in order; the fences keep the compiler from moving them) */
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        int4* out = reinterpret_cast<int4*>(a.world + (size_t)(base + i0));
        for (int j = lane; j < 6 * m; j += 64) out[j] = mine[j];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

extern "C" {

/* The arguments are checked by is_stixel_world. */
hipError_t isk_launch_world(const is_world_args* w, hipStream_t stream) {
    const int n_columns = w->n_images * w->realcols;
    hipError_t e = isk_launch_count_sections(w->d_sections, n_columns, w->max_sections, w->d_counts, w->d_offsets,
                                             stream);
    if (e != hipSuccess) return e;
    WorldArgs a;
    a.sections = w->d_sections;
    a.section_instance = w->d_section_instance;
    a.counts = w->d_counts;
    a.offsets = w->d_offsets;
    a.world = w->d_world;
    a.frame_totals = w->d_frame_totals;
    a.realcols = w->realcols;
    a.S = w->max_sections;
    a.rows = w->rows;
    a.column_step = w->column_step;
    a.capacity = w->capacity;
    a.focal = w->focal;
    a.baseline = w->baseline;
    a.cx = w->camera_center_x;
    a.cy = w->camera_center_y;
    for (int first = 0; first < w->n_images; first += IS_WORLD_IMAGES) {
        WorldRoad road = {};
        a.first_image = first;
        a.n_images = w->n_images - first < IS_WORLD_IMAGES ? w->n_images - first : IS_WORLD_IMAGES;
        for (int i = 0; i < a.n_images; i++) {
            road.alpha_ground[i] = w->h_alpha_ground[first + i];
            road.vhor[i] = w->h_vhor[first + i];
        }
        hipLaunchKernelGGL(k_world, dim3((a.n_images * a.realcols + 3) / 4), dim3(256), 0, stream, a, road);
    }
    return hipGetLastError();
}

} /* extern "C" */
