/*
 * is_launch.h -- the internal launch interface of the gfx950 column-DP core: every isk_* function, declared once and
 * included by every file that defines or calls one (a drifted definition does not compile).  None is public ABI.
 * plan_call (is_core.hip) makes every launch decision of a DP call; the DP launchers launch what its CallPlan says.
 */
#ifndef IS_LAUNCH_H_
#define IS_LAUNCH_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "instance_stixels_core.h"
#include "is_device.h"

/* ---- size thresholds of plan_call (columns of the call = n_images * realcols); -D overrides ---- */
#ifndef IS_UNARY_PATH_MIN_COLS
#define IS_UNARY_PATH_MIN_COLS 2048 /* the unary DP of the visited rows only (k_unary_path), see IS_UNARY_PATH in plan_call */
#endif
#ifndef ISF_WIN_MIN_COLS
#define ISF_WIN_MIN_COLS 0 /* columns per call from which the unary DP stages fn windows.  Round 4: 2048 (frames/s windowed | classic at batch 2: 6470 | 6050, 4: 6090 | 6350, 8: 6890 | 6680, 16: 7480 | 7010, 32: 7860 | 7200); with the diagonal blocks in quarters (round 5) the windowed launch wins at every size: batch 1: 6290 | 5220, 2: 8180 | 6140, 4: 7110 | 6380, 8: 9190 | 9070 */
#endif
#ifndef ISF_WIN_WAVES
#define ISF_WIN_WAVES 4 /* waves per workgroup of the windowed unary tiles (the fused LUT units need 4: a LUT block) */
#endif
#ifndef ISF_LUTF_MIN_COLS
#define ISF_LUTF_MIN_COLS 2048 /* columns per call from which the LUT units run inside the unary DP launch by default (frames/s fused | prepare launch at 1 / 4 / 8 / 12 / 16 / 64 frames per call: 4730 | 6240, 7070 | 7100, 9300 | 9060, 9930 | 9440, 9610 | 9100, 11 030 | 10 160) */
#endif
#ifndef IS_P1_WIN_MIN_COLS
#define IS_P1_WIN_MIN_COLS 4096 /* columns per call from which pairwise phase 1 stages fn windows: a call of a few frames does not fill the chip, there the eight waves per column are the parallelism (one frame 1.57 ms classic, 1.63 ms windowed; frames/s at batch 4 / 8 / 16 / 32: 1461 / 2068 / 2795 / 3178 classic, 1424 / 2010 / 2798 / 3269 windowed) */
#endif
#ifndef IS_PW_SPLIT_MAX_COLS
#define IS_PW_SPLIT_MAX_COLS 512 /* up to that many columns: two phase-1 workgroups per (column, tile) (measured on MI355X, frames/s of one / two 256-column frames per call: 1 workgroup per (column, tile) 540 / 903, 2: 587 / 931, 3: 584 / -, 4: 561 / -) */
#endif
static_assert(2 * IS_PW_SPLIT_MAX_COLS <= IS_PW_SPLIT_TARGET_WGS && IS_PW_MAX_SPLIT >= 2,
              "the context reserves IS_PW_SPLIT_TARGET_WGS partial-minima slots for the split phase 1");
#define IS_PAIRWISE_SPLIT_MIN_COLS 1024 /* columns per group before the pairwise DP uses one more stream */
#define IS_PAIRWISE_MAX_GROUPS 3       /* column groups (streams of the context) of the pairwise DP; IS_PW_GROUPS overrides.  The latency-bound phase 2 of one group runs beside the launches of the others.  Round 5, frames/s with 1 / 2 / 3 / 4 groups: batch 64 4116 / 4283 / 4333 / 4227, batch 32 3776 / 3909 / 4009 / 3992, batch 16 2937 / 3120 / 3147 / 3219 (profiles/r05_ab_groups.log).  Beside a PIPELINED RCCL gather of the previous step's output (bench.py --gpus N, parallel.py) the groups cost 5 % instead (round 4: 3680 against 3860): such callers create their context with IS_PW_GROUPS=1, as bench.py does */
#define IS_P2_SPLIT_MAX_COLS 2048     /* up to eight 2048-px frames: phase 2 of the pairwise DP as chain + evaluator waves per column (k_pw_phase2s): it shortens the serial chain of a column (one frame: 82 -> 74 us per tile) but spends four wave slots per column, which costs throughput at large batches (batch 64: 32.7 vs 25.4 ms per step).  IS_P2_SPLIT=0/1 overrides. */
#define IS_BACKTRACE_STAGE_MAX_COLS 2048 /* up to eight 2048-px frames: the back-trace chases in LDS */
#ifndef IS_BACKTRACE_TWO_MIN_COLS
#define IS_BACKTRACE_TWO_MIN_COLS 8192 /* two columns per wave: more one-column waves than the chip holds at once */
#endif

/* ---- one DP call ---- */

/* rows of a column's carry buffer lutC (CallPlan::lut_carry): the carries lutT[32 k] of the ceil(H / 32) LUT blocks */
__host__ __device__ inline int isk_lut_carry_rows(int H) { return (H + 31) / 32; }

enum { IS_P2_ONE = 0, IS_P2_SPLIT = 1, IS_P2_TWO = 2 };       /* k_pw_phase2 | k_pw_phase2s | k_pw_phase2x + generic */
enum { IS_BT_PLAIN = 0, IS_BT_STAGED = 1, IS_BT_TWO = 2 };    /* k_backtrace<false> | <true> | <false, true> */

/* Every launch decision of one is_compute call (plan_call, is_core.hip). */
struct CallPlan {
    int ncols;         /* columns of the call */
    int pairwise;
    int nwaves;        /* waves per DP workgroup of the classic tiles */
    int win_tiles;     /* the DP tiles 0 .. win_tiles - 1 stage an fn window (IS_P1_WIN); <= ntiles */
    /* unary */
    int unary_walk;    /* 1: k_unary_path + the generic columns + the repair launch; 0: the tile path */
    int unary_force_bad; /* (tests, IS_UNARY_PATH=3) every walk distrusts itself: the repair launch runs */
    int walk_sections; /* 1 (a walk call without instance outputs): k_unary_path writes the Sections of the columns it
                        * takes, and k_backtrace runs gated: only generic columns, every column of a distrusted call */
    int unary_nvr;     /* tile path: k_dp_unary_fast<., NVR> for the FAST columns; 0 = k_dp_unary for every column */
    int lut_fused;     /* 1: the LUT units run inside the unary DP launch (LUTF) */
    /* prepare */
    int prepare_lut;   /* 1: k_prepare_fused (records + object LUT); 0: k_prepare_columns (records only) */
    int lut_carry;     /* 1 (with unary_walk): the prepare launch stores only the LUT's block carries (lutC) */
    int lut_carry_lds; /* 1 (with lut_carry, D <= 128): k_prepare_columns + k_lut_carry, the cost table in LDS */
    /* pairwise */
    int groups;        /* column groups, one stream each */
    int nsplit;        /* phase-1 workgroups per (column, tile) */
    int phase2;        /* IS_P2_* */
    /* back-trace */
    int backtrace;     /* IS_BT_* */
};

struct StepRec;

/* The device buffers of one DP call: the context's scratch and the caller's tables. */
struct CallBuffers {
    const float* joined;
    const int32_t* seg;
    const float* ground;
    const int* vhor;
    const float* cost_T;
    const float* cost_F;
    const float* odr;
    const float* rcp;
    RowRec* recs;
    float* lutT;
    float* lutC;
    int* col_flags;
    float* sv;
    PruneRec* prune;
    int* n_generic;
    int* path_bad;
    PriorRec* priors;
    StepRec* steps;
    float* part_cost;
    int* part_idx;
    float* blksum;
    float* t8row;
    float* cost_table;
    int32_t* index_table;
    is_section* sections;      /* the caller's Section output */
    unsigned long long* counters; /* null unless the evaluation counters are on */
    int* inst_cnt;             /* null unless instance outputs are requested */
};

extern "C" {

/* is_core.hip */
int isk_fail(int code, const char* msg);

/* is_k_prepare.hip */
size_t isk_prepare_lds_bytes(const DevParams* P);
hipError_t isk_set_lds_prepare(const DevParams* P);
hipError_t isk_launch_prepare(const DevParams* P, const CallPlan* plan, const CallBuffers* b, hipStream_t stream);
hipError_t isk_launch_priors(const DevParams* P, const float* ground, PriorRec* priors, int n_images,
                             hipStream_t stream);
hipError_t isk_launch_lut_repair(const DevParams* P, int ncols, const float* joined, const float* cost_T, float* lutT,
                                 const int* run_if, hipStream_t stream);
hipError_t isk_launch_lut_generic(const DevParams* P, const CallPlan* plan, const CallBuffers* b, hipStream_t stream);
size_t isk_lut_carry_lds_bytes(const DevParams* P);
hipError_t isk_set_lds_lut_carry(const DevParams* P);
hipError_t isk_launch_lut_carry(const DevParams* P, const CallPlan* plan, const CallBuffers* b, hipStream_t stream);
int isk_lut_carry_pass_columns(void);

/* is_k_unary.hip */
size_t isk_unary_lds_bytes(const DevParams* P);
hipError_t isk_set_lds_unary(const DevParams* P);
hipError_t isk_launch_dp_unary(const DevParams* P, const CallPlan* plan, const CallBuffers* b, hipStream_t stream);
int isk_debug_occupancy(const DevParams* P, int nwaves);

/* is_k_unary_fast.hip */
size_t isk_unary_fast_lds_bytes(const DevParams* P, int nvr);
int isk_unary_fast_chunk_rows(const DevParams* P);
hipError_t isk_set_lds_unary_fast(const DevParams* P);
hipError_t isk_launch_dp_unary_fast(const DevParams* P, const CallPlan* plan, const CallBuffers* b,
                                    hipStream_t stream);

/* is_k_unary_path.hip */
size_t isk_unary_path_lds_bytes(const DevParams* P);
hipError_t isk_set_lds_unary_path(const DevParams* P);
hipError_t isk_launch_unary_path(const DevParams* P, const CallPlan* plan, const CallBuffers* b, hipStream_t stream);

/* is_k_pairwise.hip */
size_t isk_pairwise_lds_bytes(const DevParams* P, int nwaves);
size_t isk_phase2_lds_bytes(const DevParams* P);
size_t isk_phase2x_lds_bytes(const DevParams* P);
size_t isk_phase2s_lds_bytes(const DevParams* P);
hipError_t isk_set_lds_pairwise(const DevParams* P, int nwaves);
hipError_t isk_launch_dp_pairwise(const DevParams* P, const CallPlan* plan, const CallBuffers* b, hipStream_t stream,
                                  const hipStream_t* aux, hipEvent_t ev_fork, const hipEvent_t* ev_join);

/* is_k_backtrace.hip */
size_t isk_backtrace_lds_bytes(const DevParams* P, int form);
hipError_t isk_set_lds_backtrace(const DevParams* P);
hipError_t isk_launch_backtrace(const DevParams* P, const CallPlan* plan, const CallBuffers* b, hipStream_t stream);
hipError_t isk_launch_compact(const DevParams* P, int n_images, const is_section* sections, const int* inst_cnt,
                              const is_instance_buffers* d_tbl, hipStream_t stream);

/* is_k_cluster.hip */
hipError_t isk_launch_cluster(int n_slots, float eps, int min_pts, int n_images, const is_instance_buffers* d_tbl,
                              const is_instance_buffers* one, int32_t* scratch, hipStream_t stream);

/* is_k_sweep.hip: a parameter sweep (is_compute_sweep) and the re-clustering (is_recluster) */
#define IS_SWEEP_SCALE_SETS 64 /* sets per k_prune_scale launch: their factors travel as a kernel argument */
struct SweepScale { /* per set: the two weights of PruneRec and the set's object slack (+inf: pruning off) */
    float dw[IS_SWEEP_SCALE_SETS], iw[IS_SWEEP_SCALE_SETS], sigma_od[IS_SWEEP_SCALE_SETS];
};
hipError_t isk_launch_prune_scale(const PruneRec* base, PruneRec* out, int ncols, int n_sets, const SweepScale* sc,
                                  hipStream_t stream);
hipError_t isk_launch_sweep_state(int* n_generic, int* path_bad, int* saved, int restore, hipStream_t stream);
hipError_t isk_launch_recore(int n_slots, int max_sections, int size_filter, int n_images, const is_section* sections,
                             const is_instance_buffers* d_tbl, hipStream_t stream);

/* is_k_frontend.hip */
hipError_t isk_launch_join(const float* big, float* joined, int H, int W, int C, int step, int margin, int median,
                           float invalid, int n_images, hipStream_t stream);
hipError_t isk_launch_flip_and_pad(const float* in, int32_t* out, int n, int CH, int Hs, int Ws, int P2S,
                                   hipStream_t stream);

/* is_k_pack.hip */
hipError_t isk_launch_count_sections(const is_section* sections, int n_columns, int S, int32_t* counts,
                                     int32_t* offsets, hipStream_t stream);
hipError_t isk_launch_pack(const is_section* sections, int n_columns, int S, int32_t* counts, int32_t* offsets,
                           is_section* packed, hipStream_t stream);
hipError_t isk_launch_unpack(const int32_t* counts, int32_t* offsets, const is_section* packed, int n_columns, int S,
                             is_section* sections, hipStream_t stream);

/* is_k_road.hip */
int isk_road_sort_max(void);
int isk_road_counters(void);
hipError_t isk_set_lds_road_hough(int bytes);
hipError_t isk_launch_road_vdisparity(const float* disparity, int* vdisp, uint8_t* binary, int* counters, int* points,
                                      int n_images, int rows, int cols, int max_dis, float threshold,
                                      hipStream_t stream);
hipError_t isk_launch_road_vdisparity_single(const float* disparity, int* vdisp, uint8_t* binary, int* maximum,
                                             int rows, int cols, int max_dis, float threshold, hipStream_t stream);
hipError_t isk_launch_road_hough(const int* points, const int* counters, int* ncand, const float* tab, int2* cand,
                                 float* lines, int* votes, int* total, int* overflow, int n_images, int n_cells,
                                 int numangle, int numrho, int band, int threshold, int cap, int max_lines, float rho,
                                 float theta, hipStream_t stream);

hipError_t isk_launch_road_choose(const float* lines, const int* total, const int* overflow, const float* tabT,
                                  is_road_params* road, uint8_t* status, int n_images, int max_lines, int numangle,
                                  float step, int rows, float cy, float baseline, float focal, float min_pitch,
                                  float max_pitch, is_road_params fallback, hipStream_t stream);

/* is_k_ground.hip */
hipError_t isk_launch_ground_model(const is_ground_params* g, const float* log_lut, int lut_entries,
                                   const is_road_params* road, float* ground, int* vhor, int n_images, int rows,
                                   hipStream_t stream);

/* is_k_render.hip */
int isk_render_scatter_images(void);
hipError_t isk_launch_section_instance(const is_instance_buffers* per_image, int n_images, int first_image,
                                       int realcols, int max_sections, int32_t* out, hipStream_t stream);
hipError_t isk_launch_render(const is_render_args* r, const uint8_t* table, int n_classes, hipStream_t stream);

/* is_k_instance_eval.hip */
hipError_t isk_launch_instance_overlap(const is_instance_overlap_args* r, hipStream_t stream);
hipError_t isk_launch_pack_overlap(const is_overlap_record* records, const int32_t* n_records, int n_images,
                                   int capacity, is_overlap_record* packed, hipStream_t stream);

/* is_k_world.hip */
hipError_t isk_launch_world(const is_world_args* w, hipStream_t stream);

/* is_k_assign_gt.hip */
hipError_t isk_launch_assign_gt(const is_assign_gt_args* r, const int* label_ids, hipStream_t stream);
hipError_t isk_launch_pack_section_labels(const int32_t* map, int n_images, int realcols, int max_sections,
                                          int capacity, int32_t* packed, hipStream_t stream);

/* is_k_instance_disparity.hip */
size_t isk_instance_disparity_scratch_bytes(int n_images, int realcols, int max_sections, int capacity);
hipError_t isk_launch_instance_disparity(const is_instance_disparity_args* r, hipStream_t stream);

/* is_k_gt_targets.hip */
hipError_t isk_launch_mode_downsample(const void* src, int dtype, int n, int Hs, int Ws, void* dst,
                                      hipStream_t stream);
size_t isk_gt_targets_scratch_bytes(int n_images, int Hs, int Ws, int disparity, int capacity);
hipError_t isk_launch_gt_targets(const is_gt_targets_args* r, int capacity, hipStream_t stream);

/* is_k_offset_loss.hip */
size_t isk_offset_loss_scratch_bytes(int n_images, int planes, int Hs, int Ws, int capacity);
hipError_t isk_launch_offset_loss(const is_offset_loss_args* r, int capacity, hipStream_t stream);

/* is_k_head.hip */
hipError_t isk_launch_segmentation_head(const is_segmentation_head_args* a, hipStream_t stream);

/* is_k_conv3x3.hip */
hipError_t isk_launch_conv_pack(const float* d_weight, int channels_out, int channels_in, int kernel, int dtype,
                                void* d_packed, hipStream_t stream);
hipError_t isk_launch_conv_bn(const is_conv_bn_stride_args* a, hipStream_t stream);

/* is_k_conv_backward.hip */
size_t isk_conv_backward_scratch_bytes(int n_images, int channels_in, int channels_out, int rows_in, int cols_in, int kernel,
                                       int stride);
hipError_t isk_launch_conv_bn_backward(const is_conv_bn_stride_backward_args* a, hipStream_t stream);

/* ... and its two reductions on another launcher's partials (f23): part[(chunk * taps + tap) * Cout * Cin + co * Cin + ci],
 * shift_part[(image * Cout + co) * pblocks + block] */
void isk_launch_conv_bwd_reduce(const float* part, int chunks, int Cin, int Cout, int taps, const float* scale, float* dw,
                                double* gsum, hipStream_t stream);
void isk_launch_conv_bwd_channel(int dtype, const double* gsum, const float* weight, const double* shift_part, int n_images,
                                 int pblocks, int Cin, int Cout, int taps, float* dscale, float* dshift, hipStream_t stream);

/* is_k_conv_backward_stride.hip: the two stride-2 kernels of the launcher above.  gh, part: the launcher's sections. */
void isk_launch_conv_bwd_data_s2(const is_conv_bn_stride_backward_args* a, const void* gh, const void* packed,
                                 hipStream_t stream);
void isk_launch_conv_bwd_weight_s2(const is_conv_bn_stride_backward_args* a, const void* gh, float* part, hipStream_t stream);

/* is_k_stem.hip */
size_t isk_stem_packed_bytes(void);
hipError_t isk_launch_stem_pack(const float* d_w0, const float* d_w1, int dtype, void* d_packed, hipStream_t stream);
hipError_t isk_launch_stem(const is_stem_args* a, hipStream_t stream);

/* is_k_stem_backward.hip */
size_t isk_stem_backward_scratch_bytes(int n_images, int rows, int cols, int channels_next);
hipError_t isk_launch_stem_backward(const is_stem_backward_args* a, hipStream_t stream);

/* is_k_head_backward.hip */
size_t isk_head_backward_scratch_bytes(int n_images, int K, int Hs, int Ws, int channels);
hipError_t isk_launch_segmentation_head_backward(const is_segmentation_head_backward_args* a, hipStream_t stream);

/* is_k_nll.hip */
size_t isk_semantic_nll_scratch_bytes(int n_images, int Hs, int Ws);
hipError_t isk_launch_semantic_nll(const is_semantic_nll_args* a, hipStream_t stream);

/* is_k_cnn_labels.hip */
hipError_t isk_launch_cnn_labels(const is_cnn_label_args* r, const uint8_t* table, hipStream_t stream);

/* is_k_nll_up.hip */
size_t isk_semantic_nll_up_scratch_bytes(int n_images, int rows8, int cols8);
hipError_t isk_launch_semantic_nll_up(const is_semantic_nll_up_args* r, hipStream_t stream);

/* is_k_objects.hip */
hipError_t isk_launch_instance_objects(const is_instance_objects_args* r, hipStream_t stream);

} /* extern "C" */

#endif /* IS_LAUNCH_H_ */
