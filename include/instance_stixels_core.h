/*
 * instance_stixels_core.h -- C ABI of the MI355X (gfx950) Instance-Stixels column-DP core.
 *
 * This is the drop-in boundary of the hot path: plain pointers and sizes, no C++ or torch
 * types.  It is what the reference's host class `Stixels`
 * (/root/reference/InstanceStixels/include/InstanceStixels/Stixels.hpp:40-96) needs from the
 * device side: the three kernel launches of `Stixels::Compute`
 * (/root/reference/InstanceStixels/src/Stixels.cu:509-590) plus the buffer management of
 * `Stixels::Initialize` / `Finish` (Stixels.cu:43-283).  The header-compatible `Stixels`
 * class in include/InstanceStixels/Stixels.hpp is implemented only in terms of these
 * entry points.
 *
 * All functions return 0 on success and a negative IS_E* code on failure; the failing HIP
 * error string is available from is_last_error().  Nothing here falls back to a CPU path.
 */
#ifndef INSTANCE_STIXELS_CORE_H_
#define INSTANCE_STIXELS_CORE_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IS_OK 0
#define IS_EINVAL (-1)  /* bad argument / unsupported shape */
#define IS_EHIP (-2)    /* HIP runtime failure, see is_last_error() */
#define IS_ENOMEM (-3)

#define IS_GROUND 0
#define IS_OBJECT 1
#define IS_SKY 2

#define IS_DOWNSAMPLE_FACTOR 8       /* configuration.h:31 */
#define IS_MAX_STIXELS_PER_COLUMN 200 /* configuration.h:32 */
#define IS_INSTANCE_CLASSES 8        /* Stixels.cu:47 (Cityscapes classes 11..18) */
#define IS_FIRST_INSTANCE_CLASS 11   /* StixelsKernels.cu:926 */

/* Same fields, order and layout as `struct StixelParameters`
 * (/root/reference/InstanceStixels/include/InstanceStixels/types.h:145-184). */
typedef struct is_stixel_params {
    int vhor;
    int rows;
    int rows_power2;
    int rows_power2_segmentation;
    int cols; /* = realcols, Stixels.cu:213 */
    int max_dis;
    float rows_log;
    float pnexists_given_sky_log;
    float normalization_sky;
    float inv_sigma2_sky;
    float puniform_sky;
    float nopnexists_given_sky_log;
    float pnexists_given_ground_log;
    float puniform;
    float nopnexists_given_ground_log;
    float pnexists_given_object_log;
    float nopnexists_given_object_log;
    float baseline;
    float focal;
    float range_objects_z;
    float pord;
    float epsilon;
    float pgrav;
    float pblg;
    float max_dis_log;
    int max_sections;
    int width_margin;
    int segmentation_classes;
    int segmentation_channels;
    float prior_weight;
    float disparity_weight;
    float segmentation_weight;
    float instance_weight;
    int column_step;
    float clustering_eps;
    int clustering_min_pts;
    int clustering_size_filter;
    float invalid_disparity;
} is_stixel_params;

/* Same layout as `struct Section` (types.h:186-194), 32 bytes. */
typedef struct is_section {
    int type; /* IS_GROUND / IS_OBJECT / IS_SKY, -1 = terminator */
    int vB, vT;
    float disparity;
    int semantic_class;
    float cost;
    float instance_meanx;
    float instance_meany;
} is_section;

/* Device-side instance-candidate arrays of ONE image, laid out as the reference's
 * d_instance_* members (Stixels.cu:56-74; filled at StixelsKernels.cu:926-942).
 * class_offset = class_id * realcols * max_sections.  Any pointer may be NULL to skip it.
 * Order inside a class is canonical (column ascending, then section index ascending)
 * instead of the reference's atomic arrival order. */
/* ABI 0.3: the struct MUST be zero-initialised (memset / `= {}`) before its fields are set --
 * is_compute dereferences every non-NULL member, and members added by later versions then stay
 * NULL.  All calls on one context must be stream-ordered (the context owns scratch that
 * is_compute and is_cluster_instances share). */
typedef struct is_instance_buffers {
    float* d_centerofmass;     /* [8][realcols*max_sections][2]  (meanx, meany) */
    int32_t* d_indices;        /* [8][realcols*max_sections][2]  (column, section index) */
    uint8_t* d_core_candidates; /* [8][realcols*max_sections]    (bool)   */
    int32_t* d_instances_per_class; /* [8] */
    /* [8][realcols*max_sections] cluster label of every candidate (the reference's
     * d_instance_labels, Stixels.cu:660-666): 0.. per class, -1 = no instance.  NULL skips the
     * clustering; non-NULL requires the three arrays above. */
    int32_t* d_labels;
    /* optional, [1 + 3*8*realcols*max_sections]: d_packed[0] = number of candidates of all
     * classes, then one (column, section index, label) triple per candidate, classes ascending:
     * what Stixels::GetInstanceStixels (Stixels.cu:744-776) needs, in one small copy.  Written
     * together with d_labels; needs d_indices. */
    int32_t* d_packed;
} is_instance_buffers;

typedef struct is_ctx is_ctx;

/* Replaces the device half of Stixels::Initialize (Stixels.cu:53-74, 136-210): uploads the
 * frame-independent LUTs and allocates all scratch for up to `max_batch` images per call.
 *   obj_cost_lut         host, [max_dis][max_dis]   (Stixels.cu:122-129)
 *   obj_disparity_range  host, [max_dis]            (Stixels.cu:111-115)
 * `params->vhor` is ignored here (it is a per-frame value, Stixels.cu:532). */
int is_ctx_create(const is_stixel_params* params, const float* obj_cost_lut,
                  const float* obj_disparity_range, int max_batch, int device,
                  is_ctx** out_ctx);

/* Replaces Stixels::Finish (Stixels.cu:250-283). */
int is_ctx_destroy(is_ctx* ctx);

/* Replaces the JoinColumns launch (Stixels.cu:509-511, kernel StixelsKernels.cu:980-1095).
 *   d_disparity_big  device, [n_images][rows][full_cols] row-major, image row 0 = top
 *   d_joined         device, [n_images][realcols][rows], row 0 = image bottom
 * `stream` is a hipStream_t (NULL = default stream). */
int is_join_columns(is_ctx* ctx, const float* d_disparity_big, int full_cols, int median_join,
                    float* d_joined, int n_images, void* stream);

/* Replaces the ComputeObjectLUT + StixelsKernel<PAIRWISE> launches (Stixels.cu:535-590) for
 * a batch of `n_images` independent images that share the configuration of the context.
 *   d_joined            device, [n_images][realcols][rows]                 (read only)
 *   d_segmentation      device, [n_images][realcols][channels][rows_power2_segmentation]
 *                       int32, layout of tools/CNN_training/models/wrappers.py:35-61.  Read
 *                       only: unlike the reference the input is NOT modified.
 *   h_ground_function, h_normalization_ground, h_inv_sigma2_ground
 *                       host, [n_images][rows]  (Stixels::PrecomputeGround, Stixels.cu:790-817)
 *   h_vhor              host, [n_images], library convention rows-vhor_image-1 (Stixels.cu:377)
 *   d_sections          device, [n_images][realcols][max_sections] is_section
 *   instances           per image (array of n_images) or NULL.  The candidates of the whole
 *                       batch are compacted by ONE launch and clustered by ONE launch
 *                       (grid = 8 classes x n_images), whatever n_images is.
 *   d_cost_table        optional device out, [n_images][realcols][rows][3] final DP costs
 *   d_index_table       optional device out, [n_images][realcols][rows][3] int32.  PAIRWISE:
 *                       vB*3 + predecessor type, the reference's encoding
 *                       (StixelsKernels.cu:723-727).  UNARY: the winning vB only (-1 = no
 *                       candidate) -- in unary mode the predecessor type depends only on the
 *                       final cost_table[vB-1] and is resolved by the back-trace,
 *                       so decoding a unary table with /3 and %3 is WRONG.
 * Alignment: d_joined and d_segmentation are read with 16-byte vector loads; both must be
 * 16-byte aligned (any hipMalloc / torch allocation is) -- checked, IS_EINVAL otherwise.
 * Device: the call runs on the context's device whatever the caller's current device is (the
 * current device is restored on return); `stream` must belong to that device.
 * Asynchronous with respect to the host: work is queued on `stream`; the host arrays are copied
 * into a ring of pinned staging slots before the call returns.
 * Internal invariant: the context's generic-column counter is zero between calls (counted by the
 * prepare kernel, cleared by the back-trace at the end of the call); a call that returns an error
 * clears it itself. */
int is_compute(is_ctx* ctx, const float* d_joined, const int32_t* d_segmentation,
               const float* h_ground_function, const float* h_normalization_ground,
               const float* h_inv_sigma2_ground, const int* h_vhor, int pairwise,
               int n_images, is_section* d_sections, const is_instance_buffers* instances,
               float* d_cost_table, int32_t* d_index_table, void* stream);

/* ---- the ground model of a batch on the device (k_ground_model, is_k_ground.hip) -------------------------------
 * The constants of Stixels::PrecomputeGround, as the host class holds them (sigma_camera_tilt in radians). */
typedef struct is_road_params { /* one frame's road, the layout of Stixels::RoadParameters (16 bytes) */
    int vhor;                   /* image-convention horizon row */
    float tilt, height, alpha;  /* camera pitch and height, slope of the ground line in the v-disparity image */
} is_road_params;
typedef struct is_ground_params {
    float focal, baseline;
    float max_dis; /* (float)max_dis */
    float pout;
    float sigma_disparity_ground, sigma_camera_height, sigma_camera_tilt;
} is_ground_params;

/* Stores the constants and uploads the table Stixels::FastLog reads (h_log_lut [n_entries] float, n_entries >= 2:
 * entry i = logf(i / (n_entries - 1)); the host class has 10^6 + 1) once per context; synchronous.  Needed before
 * is_compute_road; may be called again. */
int is_ctx_set_ground_model(is_ctx* ctx, const is_ground_params* params, const float* h_log_lut, int n_entries);

/* is_compute with the ground model of every frame built on the device from d_road [n_images] (is_road_params, device;
 * e.g. what is_road_choose_batch left): k_ground_model writes the context's ground arrays and horizons -- row for row
 * is_ground_row of is_ground_model.h, i.e. Stixels::PrecomputeGroundShared, bitwise -- and then exactly the launches
 * of is_compute follow.  Nothing of the ground model crosses the host; the instance table is staged as in is_compute.
 *   vhor_min_hint   < 0: unknown; else a lower bound of the library-convention horizons (rows - vhor - 1) of the
 *                   call.  Launch geometry only (how many pairwise tiles stage an fn window), never results.
 * Every other argument and constraint as is_compute. */
int is_compute_road(is_ctx* ctx, const float* d_joined, const int32_t* d_segmentation, const is_road_params* d_road,
                    int pairwise, int n_images, is_section* d_sections, const is_instance_buffers* instances,
                    float* d_cost_table, int32_t* d_index_table, int vhor_min_hint, void* stream);

/* (tests) the ground model of frame `frame` of the last compute call as the DP kernels read it: h_out [3][rows]
 * (function, normalization, inv_sigma2) and its library-convention horizon; synchronises the device. */
int is_debug_read_ground(is_ctx* ctx, int frame, float* h_out, int* vhor);

/* Replaces Stixels::ClusterInstances (Stixels.cu:639-681: one ML::dbscanFit per instance class
 * with the size filter of the cuML fork) for the candidates of ONE image (is_compute clusters a
 * whole batch in one launch): size-filtered DBSCAN
 * with the semantics of the reference's Python twin
 * (tools/visualization/clustering_visualization.py:894-960) on the device, no host round trip.
 * Reads d_centerofmass / d_core_candidates / d_instances_per_class, writes d_labels.
 * is_compute() runs it by itself for every image whose d_labels is set. */
int is_cluster_instances(is_ctx* ctx, const is_instance_buffers* instances, void* stream);

/* ---- parameter sweeps: many weight / clustering sets on one resident batch ------------------------------------
 * The reference's hyper-parameter search (tools/run_cityscapes.py:566-680) re-runs the stixel stage over the same
 * frames while only the four weights and the three clustering parameters change.  One set of those seven: */
typedef struct is_sweep_set {
    float prior_weight, disparity_weight, segmentation_weight, instance_weight; /* as in is_stixel_params:
                                                    instance_weight already relative to segmentation_weight */
    float clustering_eps; int clustering_min_pts, clustering_size_filter; int reserved; /* 0 */
} is_sweep_set;

/* is_compute for n_sets parameter sets on the same inputs in one call.  Slice k of every output ([n_sets][n_images]
 * ...) holds, byte for byte up to each column's terminator, what is_compute writes on a context created with the same
 * is_stixel_params except the seven fields of h_sets[k].  The weight-independent work of a call (staging, column
 * records, object table, pairwise priors) runs once; the DP, the back-trace, the instance candidates and their
 * clustering run per set.  No cost / index tables.  The context's own parameters are untouched: an is_compute
 * afterwards gives what it gave before.  Asynchronous and stream-ordered like is_compute; the same constraints, and
 *   n_sets >= 1, every reserved field 0, n_sets * n_images * realcols * max_sections < 2^31
 *   d_sections   device, [n_sets][n_images][realcols][max_sections]
 *   instances    [n_sets][n_images] or NULL */
int is_compute_sweep(is_ctx* ctx, const float* d_joined, const int32_t* d_segmentation,
                     const float* h_ground_function, const float* h_normalization_ground,
                     const float* h_inv_sigma2_ground, const int* h_vhor, int pairwise, int n_images,
                     const is_sweep_set* h_sets, int n_sets, is_section* d_sections,
                     const is_instance_buffers* instances, void* stream);

/* The clustering of a compute call again with other parameters, without its DP: the core-candidate flags of every
 * candidate are derived anew from d_indices -> d_sections ((vT + 1 - vB) >= size_filter), then the batch is clustered
 * with (eps, min_pts) in one launch.  d_sections and instances [n_images] are those of the compute call (or of one
 * set of a sweep); d_labels (and d_packed, where given) afterwards equal those of a compute call made with the three
 * parameters.  Every image needs d_indices, d_centerofmass, d_core_candidates, d_instances_per_class and d_labels
 * (IS_EINVAL otherwise); n_images <= max_batch. */
int is_recluster(is_ctx* ctx, const is_section* d_sections, int n_images, float eps, int min_pts, int size_filter,
                 const is_instance_buffers* instances, void* stream);

/* Compaction of the fixed-stride Section output for the final gather of a multi-GPU batch
 * (the reference copies all max_sections = 200 slots of every column to the host,
 * Stixels.cu:629-633, of which 10-40 are used).  On the current device, on `stream`:
 *   d_sections  [n_columns][max_sections] (n_columns = n_images * realcols), terminator type -1
 *   d_counts    [n_columns]      sections in front of each column's terminator
 *   d_offsets   [n_columns + 1]  exclusive prefix of the counts; d_offsets[n_columns] = total
 *   d_packed    [>= total]       the sections in (image, column, section) order
 * is_unpack_sections is the inverse (it recomputes d_offsets from d_counts and writes the
 * terminators); entries behind a terminator are unspecified on both sides.  The d_counts given to
 * is_unpack_sections must be those is_pack_sections produced (0 <= count < max_sections, d_packed
 * holding their sum): other counts give offsets outside d_packed. */
int is_pack_sections(const is_section* d_sections, int n_columns, int max_sections,
                     int32_t* d_counts, int32_t* d_offsets, is_section* d_packed, void* stream);
int is_unpack_sections(const int32_t* d_counts, int32_t* d_offsets, const is_section* d_packed,
                       int n_columns, int max_sections, is_section* d_sections, void* stream);

/* ---- multi-GPU: the final gather of a sharded batch for C / C++ callers ----------------
 * Images are independent: every rank (one process per GPU) runs is_compute on its shard of the batch and
 * only the OUTPUT travels, to one rank, over RCCL (/opt/rocm/include/rccl/rccl.h:700-745).  `comm` is an
 * ncclComm_t passed as void*; a caller that has rccl.h uses its own communicator, a plain-C++ caller the
 * four helpers below.  RCCL is loaded at run time (dlopen of librccl.so.1): IS_EHIP if it is missing.
 * There is no reference counterpart: the reference runs on one GPU and writes its Sections to a file
 * per frame (apps/run_cityscapes.cu:430-449). */
int is_comm_unique_id(void* id_out, size_t id_bytes);  /* ncclGetUniqueId; id_bytes >= 128; pass the bytes to every rank */
int is_comm_init_rank(void** comm, int nranks, const void* id, int rank); /* ncclCommInitRank on the current device */
int is_comm_destroy(void* comm);
int is_comm_rank(void* comm, int* rank, int* nranks);
/* Gather of int32 payloads of different sizes on rank `dst`: rank r sends h_counts[r] elements of d_send;
 * dst receives them into d_recv in rank order (its own part is a device copy).  h_counts has one entry per
 * rank; a sender reads only its own.  Grouped ncclSend / ncclRecv on `stream`, asynchronous. */
int is_gather_i32(void* comm, int dst, const int64_t* h_counts, const int32_t* d_send, int32_t* d_recv,
                  void* stream);
/* The compacted gather: what is_pack_sections left on every rank goes to `dst`.
 *   h_columns      host, [nranks]: columns (n_images * realcols) of every rank's shard -- the shard sizes are
 *                  known everywhere (contiguous blocks of the batch); the same array on every rank
 *   d_counts, d_offsets, d_packed   this rank's is_pack_sections output (d_offsets[columns] = its total)
 *   d_all_counts   dst: [sum of h_columns], rank order
 *   d_all_packed   dst: [cap_sections] is_section, the ranks' sections back to back in rank order
 *   h_totals       host, [nranks], out: on dst the sections of every rank, elsewhere only entry [own rank]
 * Two phases on `stream`: the sizes (ncclGather) and the per-column counts, a host synchronisation, dst's
 * go-ahead (IS_ENOMEM on EVERY rank when the total exceeds cap_sections: nothing is sent), then the payload
 * (queued; the caller synchronises `stream`).  is_unpack_sections on dst restores the fixed-stride arrays. */
int is_gather_sections(void* comm, int dst, const int32_t* h_columns, const int32_t* d_counts,
                       const int32_t* d_offsets, const is_section* d_packed, int32_t* d_all_counts,
                       is_section* d_all_packed, size_t cap_sections, int64_t* h_totals, void* stream);

/* Replaces the output wrapper of the reference's CNN export ("FlipAndPad",
 * tools/CNN_training/models/wrappers.py:35-61), i.e. the producer of d_segmentation:
 *   d_cnn_out       device, [n_images][channels][rows8][cols8] float (NCHW network output)
 *   d_segmentation  device, [n_images][cols8][channels][rows_power2_segmentation] int32:
 *                   permuted, rows flipped (index 0 = image bottom), zero padded, (int)(8*x). */
int is_flip_and_pad(const float* d_cnn_out, int32_t* d_segmentation, int n_images, int channels,
                    int rows8, int cols8, int rows_power2_segmentation, void* stream);

/* Replaces the three launches of RoadEstimation::Compute (RoadEstimation.cu:103-118, kernels
 * RoadEstimationKernels.cu:25-60): v-disparity histogram of the full-resolution disparity image
 * (pixels equal to 0 are skipped), its maximum, and the binarised image
 * (count > maximum * threshold ? 255 : 0).
 *   d_disparity [rows][cols] float;  d_vdisp [rows][max_dis] int;  d_maximum [1] int;
 *   d_binary [rows][max_dis] uint8. */
int is_road_vdisparity(const float* d_disparity, int rows, int cols, int max_dis, float threshold,
                       int* d_vdisp, int* d_maximum, uint8_t* d_binary, void* stream);

/* ---- batched road estimation: is_road_vdisparity + RoadEstimation::HoughLines for n frames ----------------
 * Every launch covers the whole batch (the number of launches does not depend on n), and every result is
 * bitwise the one of the single-frame path: the histogram, maximum and binary image of is_road_vdisparity, and
 * the lines of RoadEstimation::HoughLines (rho = 1, theta = (float)pi / 180; sin / cos tables computed on the
 * host exactly as HoughLines computes them and uploaded once).  Nothing here falls back to the CPU.
 * A context owns the Hough tables and the scratch of up to max_batch frames of one shape.  Its calls are
 * stream-ordered like those of is_ctx: is_road_hough_batch reads what the last is_road_vdisparity_batch on
 * the same context left, so both go to one stream (or are ordered by the caller). */
typedef struct is_road_ctx is_road_ctx;

/* Largest max_candidates of is_road_hough_batch. */
#define IS_ROAD_MAX_CANDIDATES 8192

/* rows in [1, 32767], cols >= 1, max_dis in [1, 16384], max_batch >= 1; device: a HIP device index, or -1 for
 * the calling thread's current device.  Every later call on the context runs on that device and puts the
 * caller's current device back. */
int is_road_ctx_create(is_road_ctx** ctx, int rows, int cols, int max_dis, int max_batch, int device);
int is_road_ctx_destroy(is_road_ctx* ctx);
int is_road_ctx_device(const is_road_ctx* ctx);
/* The context's binary images, [max_batch][rows][max_dis] uint8 on its device: what the last
 * is_road_vdisparity_batch wrote for frame i starts at i * rows * max_dis. */
const uint8_t* is_road_ctx_binary(const is_road_ctx* ctx);

/* v-disparity of n_images frames (1 <= n_images <= max_batch) on `stream`:
 *   d_disparity  [n_images][rows][cols] float, device (pixels equal to 0 are skipped; bins outside
 *                [0, max_dis) are ignored)
 *   threshold    binarisation: count > maximum * threshold ? 255 : 0 (fp32, as is_road_vdisparity)
 *   d_vdisp      optional (may be null), device [n_images][rows][max_dis] int: the histograms
 *   d_maximum    optional, device [n_images] int: the maximum of each histogram
 *   d_binary     optional, device [n_images][rows][max_dis] uint8: the binary images
 * The context keeps the binary images and the list of non-zero pixels of each frame for is_road_hough_batch;
 * the optional outputs are copies of its scratch. */
int is_road_vdisparity_batch(is_road_ctx* ctx, const float* d_disparity, int n_images, float threshold,
                             int* d_vdisp, int* d_maximum, uint8_t* d_binary, void* stream);

/* Standard Hough transform of the binary images of the last is_road_vdisparity_batch (n_images no more than
 * that call's) on `stream`: accumulator threshold `threshold` (votes > threshold), 4-neighbour local maxima
 * with HoughLines' comparisons, lines sorted by votes descending, then accumulator index ascending.
 *   max_lines       >= 1: lines written per frame
 *   max_candidates  [1, IS_ROAD_MAX_CANDIDATES]: local maxima kept per frame for the sort
 *   d_lines         device [n_images][max_lines][2] float: (rho, theta) of the first min(max_lines, total)
 *                   lines, as HoughLines returns them; the rest is left as it was
 *   d_votes         optional (may be null), device [n_images][max_lines] int: the votes of those lines
 *   d_total         device [n_images] int: the number of local maxima of the frame (HoughLines' line count)
 *   d_overflow      device [n_images] int: 1 if total > max_candidates -- then the lines are NOT those of
 *                   HoughLines (the sort saw only some of the maxima), else 0 */
int is_road_hough_batch(is_road_ctx* ctx, int n_images, int threshold, int max_lines, int max_candidates,
                        float* d_lines, int* d_votes, int* d_total, int* d_overflow, void* stream);

/* ---- the road parameters of a batch chosen on the device, and the ground model built from them ----------------
 * One road record per frame, in the layout of Stixels::RoadParameters (16 bytes): the image-convention horizon row,
 * the camera pitch and height, and the slope of the ground line in the v-disparity image (is_road_params, above). */

/* d_status of is_road_choose_batch */
#define IS_ROAD_NONE 0      /* no line was accepted, and the device saw every line (total <= max_lines, no overflow) */
#define IS_ROAD_OK 1        /* a line was accepted */
#define IS_ROAD_UNDECIDED 2 /* the kept lines do not decide it: the candidate buffer overflowed (the lines are not
                             * HoughLines' then, none is looked at), or total > max_lines and no kept line was
                             * accepted -- where RoadEstimation::ComputeBatch re-runs HoughLines on the binary image */
#define IS_ROAD_HORIZON 3   /* a line was accepted, but its horizon row lies outside [0, rows) */

/* The line choice of RoadEstimation::ComputeHough for every frame, on `stream`, behind is_road_hough_batch: the
 * first line in sorted order whose pitch lies in [min_pitch, max_pitch], with rho = |rho|, evaluated by
 * the function is_road_line of is_ground_model.h -- bitwise RoadEstimation::ChooseLineShared.  One wave per frame.
 *   d_lines, d_total, d_overflow   as is_road_hough_batch wrote them for the same max_lines (device)
 *   cy, baseline, focal            the camera (RoadEstimation::Initialize); the v-disparity image has ctx rows
 *   fallback                       the record every frame whose status is not IS_ROAD_OK receives, so that whatever
 *                                  consumes d_road runs on defined numbers (a calibration, the last good frame)
 *   d_road   [n_images] is_road_params, d_status [n_images] uint8 (IS_ROAD_*), device
 * A line whose theta is not one of the transform's angles (0.0f + n * theta_step bitwise) is skipped: sin and cos
 * of the angle come from a table of the host's sinf / cosf, computed at is_road_ctx_create. */
int is_road_choose_batch(is_road_ctx* ctx, int n_images, const float* d_lines, const int* d_total,
                         const int* d_overflow, int max_lines, float cy, float baseline, float focal,
                         float min_pitch, float max_pitch, is_road_params fallback, is_road_params* d_road,
                         uint8_t* d_status, void* stream);

/* ---- f5: stixels to dense result maps, scored against ground truth on the device ----------------------------
 * The reference evaluates stixels through per-pixel images drawn on the host
 * (tools/visualization/clustering_visualization.py draw_stixels :164-413, draw_instance_masks :118-142) and
 * scores those (cityscapesscripts for the labelIds, tools/evaluation/disparity.py for the disparity).  Geometry
 * of that tooling: the stixel width is w = cols / realcols (integer division, :186 -- not column_step);
 * section (c, i) covers x in [c*w, c*w + w-1] and y in [rows-1-vT, rows-1-vB] (:214-217), inclusive.  Pixels
 * no section covers (x >= realcols*w, rows after an early terminator) are 0 in every image (:1166-1176).
 * Well-formed sections (what is_compute leaves) partition each column; hand-built ones that overlap (the
 * highest section index wins), have vB > vT or leave [0, rows-1] are clipped to the frame and never written
 * outside it. */

/* Largest n_labels of the confusion matrix, largest n_classes of a caller's class -> label table. */
#define IS_RENDER_MAX_LABELS 64
#define IS_RENDER_MAX_CLASSES 256

/* Zero-initialise (memset / `= {}`) before setting fields, as is_instance_buffers.  Every output is optional
 * (NULL: skipped, costs nothing); all device arrays are on the current device.
 *   d_sections          [n_images][realcols][max_sections] is_section, terminator type == -1 (16-byte aligned)
 *   d_section_instance  optional [n_images][realcols][max_sections] int32: the cluster label of every section,
 *                       -1 = none (is_section_instance_labels); NULL: no section is an instance
 *   rows, cols          the image (cols >= realcols); max_sections in [1, 32767]
 *   h_class_to_label    host [n_classes] (n_classes in [1, IS_RENDER_MAX_CLASSES]): semantic class -> label
 *                       value; NULL: Cityscapes trainId -> labelId (:396-402, trainId2label[c].id), n_classes
 *                       ignored.  A class outside the table gives 0.
 *   d_label             [n_images][rows][cols] uint8: the label of the covering section
 *   d_disparity         [n_images][rows][cols] float: its disparity, bit for bit, every section type (:403-409)
 *   d_instance          [n_images][rows][cols] int32: semantic_class*1000 + l for a section with cluster label
 *                       0 <= l < 1000 (read_stixel_file :108-114), else 0; the mask of instance k in
 *                       draw_instance_masks is exactly instance == k
 *   d_gt_label, d_confusion   both or neither: gt [n_images][rows][cols] uint8; confusion [n_labels][n_labels]
 *                       uint64 (n_labels in [1, IS_RENDER_MAX_LABELS]), ADDED to: conf[gt][pred] += 1 for every
 *                       pixel with gt < n_labels and pred < n_labels, pred = the label image's value (0 where no
 *                       section covers), summed over the batch
 *   d_gt_disparity, d_disp_abs_sum, d_disp_count   all or none: gt [n_images][rows][cols] float; per frame the
 *                       sum of fabsf(stixel - gt) (each term fp32, accumulated in fp64, the same bits on every
 *                       run) and the count over pixels with stixel != 0 and gt != 0 (disparity.py:56-62)
 *   d_stixel_count      [n_images] int32: sections in front of the terminators (run_cityscapes.py:611) */
typedef struct is_render_args {
    const is_section* d_sections;
    const int32_t* d_section_instance;
    int n_images, realcols, max_sections, rows, cols;
    const uint8_t* h_class_to_label;
    int n_classes;
    uint8_t* d_label;
    float* d_disparity;
    int32_t* d_instance;
    const uint8_t* d_gt_label;
    int n_labels;
    unsigned long long* d_confusion;
    const float* d_gt_disparity;
    double* d_disp_abs_sum;
    int64_t* d_disp_count;
    int32_t* d_stixel_count;
} is_render_args;

/* The per-candidate cluster labels of an is_compute call with instances (d_indices, d_labels,
 * d_instances_per_class of per_image[0 .. n_images-1]) as a per-section map: d_section_instance
 * [n_images][realcols][max_sections] int32, -1 where a section is no candidate.  On `stream`. */
int is_section_instance_labels(const is_instance_buffers* per_image, int n_images, int realcols, int max_sections,
                               int32_t* d_section_instance, void* stream);
/* Renders and scores n_images frames on `stream`, asynchronously (two launches, plus one for the label map of
 * the caller's instances above). */
int is_render_sections(const is_render_args* args, void* stream);

/* ---- f6: the instance image against ground-truth instanceIds, as a sparse joint histogram per frame ----------
 * The reference scores instances with cityscapesscripts' evalInstanceLevelSemanticLabeling, which reads one mask
 * per predicted instance (draw_instance_masks) and the *_gtFine_instanceIds.png files.  Every quantity of that
 * evaluation (areas, intersections, void and group overlaps) is a sum over the joint histogram
 *     H_f(p, g) = #{ pixels x : P_f(x) == p and G_f(x) == g },   over every pixel, p = 0 included,
 * where P_f is the instance image that is_render_sections draws -- class*1000 + l, else 0, with the same geometry
 * and clipping, built from the Sections and never read from a rendered image -- and G_f the caller's instanceIds.  The table of a
 * frame holds the non-zero entries, ascending by pred then gt (both as signed int32), and sums to rows*cols. */
typedef struct is_overlap_record {
    int32_t pred;
    int32_t gt;
    int64_t count;
} is_overlap_record;

/* Largest capacity and frame (rows * cols) of is_instance_overlap. */
#define IS_OVERLAP_MAX_CAPACITY (1 << 28)

/* Zero-initialise before setting fields.  All device arrays are on the current device.
 *   d_sections, d_section_instance, n_images, realcols, max_sections, rows, cols   as in is_render_args; the map
 *                       may be NULL, then P_f is 0 everywhere; rows * cols <= IS_OVERLAP_MAX_CAPACITY
 *   d_gt_instance       [n_images][rows][cols] int32 Cityscapes instanceIds (labelId*1000 + k, or a labelId);
 *                       any value is accepted
 *   capacity            records per frame, in [1, IS_OVERLAP_MAX_CAPACITY]; rows * cols always suffices
 *   d_records           [n_images][capacity] records, 8-byte aligned: frame f's table in its first
 *                       n_records[f] entries; the rest is left as it was
 *   d_n_records         [n_images] int32
 *   d_overflow          [n_images] int32: 1 where the frame has more than `capacity` distinct pairs; its
 *                       n_records is then 0 and its records unspecified (never written outside its row) */
typedef struct is_instance_overlap_args {
    const is_section* d_sections;
    const int32_t* d_section_instance;
    int n_images, realcols, max_sections, rows, cols;
    const int32_t* d_gt_instance;
    int capacity;
    is_overlap_record* d_records;
    int32_t* d_n_records;
    int32_t* d_overflow;
} is_instance_overlap_args;

/* The tables of n_images frames on `stream`, asynchronously (a temporary per-frame hash of 2 x capacity slots,
 * rounded up to a power of two, from the stream-ordered allocator). */
int is_instance_overlap(const is_instance_overlap_args* args, void* stream);
/* The records of is_instance_overlap's output packed back to back in frame order, frame f's n_records[f] first
 * entries of d_records [n_images][capacity] -> d_packed [sum of n_records].  On `stream`. */
int is_pack_overlap_records(const is_overlap_record* d_records, const int32_t* d_n_records, int n_images,
                            int capacity, is_overlap_record* d_packed, void* stream);

/* ---- f7: the 3-D stixel world of a batch, one record per stixel (is_k_world.hip) ------------------------------
 * What the reference's live path hands on per frame (apps/stixels_node.cu:74-208: Compute -> GetInstanceStixels ->
 * Get3DVertices -> populateStixelsArray): the fields of its InstanceStixel message plus what SaveStixels writes, for
 * every section in front of a column's terminator, in (image, column, section) order.  96 bytes = six 16-byte
 * chunks; the device writes a record as 16-byte stores, so d_world must be 16-byte aligned (the struct itself has
 * the natural alignment of its 4-byte fields; hipMalloc, pinned and numpy allocations all qualify). */
typedef struct is_world_stixel {
    int32_t column, section;   /* stixel column of its frame; index inside the column */
    int32_t type, vB, vT, semantic_class;
    int32_t instance_id;       /* the d_section_instance value, -1 = none (also with a NULL map) */
    float disparity, cost, instance_meanx, instance_meany;
    float vertices[12];        /* Get3DVertices order: TL, TR, BR, BL, each (x, y, z) */
    int32_t reserved;          /* 0 */
} is_world_stixel;
#ifdef __cplusplus
static_assert(sizeof(is_world_stixel) == 96, "is_world_stixel is six 16-byte chunks");
#else
_Static_assert(sizeof(is_world_stixel) == 96, "is_world_stixel is six 16-byte chunks");
#endif

/* Zero-initialise before setting fields.  All device arrays are on the current device.
 *   d_sections, d_section_instance, n_images, realcols, max_sections   as in is_render_args, with max_sections in
 *                       [2, 32767] and n_images * realcols * max_sections < 2^31; the map may be NULL
 *   rows, column_step   of the frame (Get3DVertices: x = column * column_step, y from rows)
 *   focal, baseline, camera_center_x, camera_center_y   the camera of SetCameraParameters
 *   h_alpha_ground, h_vhor   host [n_images]: the road of every frame, vhor in the library's convention
 *                       (StixelsData::vhor); read before the call returns
 *   capacity            records d_world holds (>= 0; d_world may be NULL when it is 0)
 *   d_counts            [n_columns] (n_columns = n_images * realcols), d_offsets [n_columns + 1]: exactly what
 *                       is_pack_sections writes there -- d_offsets[n_columns] is the TRUE total of the batch
 *   d_frame_totals      [n_images] records of every frame
 *   d_world             record r of the batch at index r for r < capacity; nothing is written at or beyond
 *                       `capacity`, the caller sees the overflow in the total and repeats
 * The records are those of the sections is_pack_sections packs.  vertices: the fp32 expressions of
 * Stixels::Get3DVertices (reference Stixels.cu:683-742) in its operand order: sky keeps depth 0, a zero
 * disparity (an object's, or ground at vhor) gives the host's +-inf, and NaN where the host has NaN. */
typedef struct is_world_args {
    const is_section* d_sections;
    const int32_t* d_section_instance;
    int n_images, realcols, max_sections, rows, column_step;
    float focal, baseline, camera_center_x, camera_center_y;
    const float* h_alpha_ground;
    const int* h_vhor;
    int capacity;
    int32_t* d_counts;
    int32_t* d_offsets;
    int32_t* d_frame_totals;
    is_world_stixel* d_world;
} is_world_args;

/* The world of n_images frames on `stream`, asynchronously: no host synchronisation, no allocation (two launches
 * for the counts and offsets, one per 64 frames for the records). */
int is_stixel_world(const is_world_args* args, void* stream);

/* ---- f8: instance ids from the ground-truth instance image, by majority vote (is_k_assign_gt.hip) -------------
 * Replaces the second way the reference's evaluation tooling gives a stixel its instance id: assign_instances_gt
 * (tools/visualization/clustering_visualization.py:846-891, option --use-instancegt of tools/run_cityscapes.py)
 * over the per-class masks of load_instance_mask (tools/visualization/cityscapes_instance_loader.py:32-71), the
 * upper-bound rows of its instance evaluation.  For every section in front of a column's terminator, whatever its
 * type, with semantic class c and w = cols / realcols (integer division):
 *   - c outside 11..18: -1.  Class c owns the labelId L = label_ids[c - 11] (c itself with gt_is_train_ids).
 *   - the rectangle is image rows rows-1-vT .. rows-1-vB, image columns column*w .. column*w + w-1, clipped to the
 *     frame in 64-bit arithmetic as is_render_sections clips (nothing outside the image is ever read; parity with
 *     the reference is claimed for sections inside the frame); an empty rectangle gives -1.
 *   - a pixel v votes for k = v - L*1000 if v > 1000 and L*1000 <= v < (L+1)*1000 (k in 0..999, the group id
 *     L*1000 is k = 0); every other pixel -- other classes, ids <= 1000, negative or huge values -- votes for
 *     background.  The most frequent value wins, background competes; ties go to background, then to the smaller
 *     k (numpy's bincount().argmax()).
 *   - the winner's pixel count must NOT be < (min_fraction * w) * (vT - vB), evaluated in binary64 in that order
 *     without contraction -- vT - vB of the section as it stands, not its height, so a one-row stixel always
 *     passes (the reference's quirk, :881-883).
 *   - the label is k when a non-background value won and passed, else -1: the consumers turn it into the instance
 *     image value c*1000 + k exactly as they do with cluster labels.
 * Slots at and behind the terminator get -1, as is_section_instance_labels leaves them.
 *
 * Zero-initialise before setting fields.  All device arrays are on the current device.
 *   d_sections, n_images, realcols, max_sections, rows, cols   as in is_render_args; rows * (cols / realcols) and
 *                       n_images * ceil(realcols / 4) must fit 31 bits
 *   d_gt_instance       [n_images][rows][cols] int32 (4-byte aligned; 16-byte aligned with cols % 8 == 0 and
 *                       w == 8 takes the vector path); any value is accepted
 *   min_fraction        0 (the zero-initialised struct) selects the reference's 0.1; a negative value switches the
 *                       rule off; NaN is refused
 *   h_label_ids         host [8] labelIds of classes 11..18, each in [0, 2147482]; NULL: Cityscapes
 *                       {24, 25, 26, 27, 28, 31, 32, 33} (*_instanceIds.png).  Read before the call returns.
 *   gt_is_train_ids     != 0: the ground truth holds c*1000 + k already (*_instanceTrainIds.png): L = c,
 *                       h_label_ids is ignored
 *   d_section_instance  [n_images][realcols][max_sections] int32, every slot written
 *   d_section_votes     optional, same shape: the winner's pixel count (background's when background won, also
 *                       when the rule rejected it), 0 where no vote took place */
typedef struct is_assign_gt_args {
    const is_section* d_sections;
    const int32_t* d_gt_instance;
    int n_images, rows, cols, realcols, max_sections;
    double min_fraction;
    const int* h_label_ids;
    int gt_is_train_ids;
    int32_t* d_section_instance;
    int32_t* d_section_votes;
} is_assign_gt_args;

/* The map of n_images frames on `stream`, asynchronously: one launch, no allocation, copy or synchronisation. */
int is_assign_instances_gt(const is_assign_gt_args* args, void* stream);
/* The labelled slots (>= 0) of a per-section map [n_images][realcols][max_sections] for one small copy to the host:
 * d_packed [4 + 4 * capacity] int32, 16-byte aligned: d_packed[0] = the number of labelled slots (the TRUE number,
 * also beyond capacity), [1..3] = 0, then one (frame, column, section, label) quad per labelled slot, at most
 * `capacity` of them, in no particular order.  n_images * realcols * max_sections < 2^31.  On `stream`. */
int is_pack_section_labels(const int32_t* d_section_instance, int n_images, int realcols, int max_sections,
                           int capacity, int32_t* d_packed, void* stream);

/* ---- f10: instance ids by clustering in (x, y, instance disparity) (is_k_instance_disparity.hip) -----------------
 * Replaces the third way the reference's evaluation tooling gives a stixel its instance id: --use-disparity from_gt
 * of tools/visualization/clustering_visualization.py, its "what if depth separated the instances" row between the
 * CNN-offset clustering (is_recluster) and the ground-truth upper bound (is_assign_instances_gt).  Per frame, with
 * w = cols / realcols (integer division):
 *   1. instance medians (compute_instance_disparity :1024-1049 over the masks of load_instance_mask,
 *      cityscapes_instance_loader.py:32-71): a ground-truth pixel id has a key when id > 1000 and id / 1000 is one of
 *      the Cityscapes labelIds 24, 25, 26, 27, 28, 31, 32, 33 (classes 11..18); key = class index * 1000 + id % 1000,
 *      8 * 1000 of them, and instance number 0 (labelId * 1000) is a key like any other.  The median of a key is
 *      np.median of the NON-ZERO disparity_u8 values under its pixels -- the two middle values of an even count
 *      averaged, so an integer number of half units in [2, 510] -- or 0 where it has none.  Every other pixel has no
 *      key and the instance disparity 0.
 *   2. stixel medians (add_instance_disparity :996-1022): for a section in front of its column's terminator with
 *      semantic class 11..18, over the rectangle of is_assign_instances_gt (image rows rows-1-vT .. rows-1-vB, image
 *      columns column*w .. column*w + w-1, clipped to the frame), the median of the pixels' instance disparities that
 *      are not < 1, the middle pair averaged: an integer number of quarter units, exact in fp32; 0 where nothing is
 *      left, for an empty rectangle, and for every other slot.
 *   3. clustering (get_disparity_instance_centers :794-819, assign_instances :894-960 with use_instance_disparity):
 *      per class, the points are the candidates whose stixel median is not 0, in candidate order; the others take no
 *      part -- they do not count towards #large > min_pts, are never core or neighbour, and get the label -1.  Over
 *      the points the rules of is_cluster_instances hold with dx*dx + dy*dy + dz*dz (fp32, no contraction, z the stixel
 *      median) against eps*eps; the core-candidate flag is (vT + 1 - vB) >= size_filter, derived as is_recluster does.
 * d_labels, d_core_candidates and d_packed (where given) of every frame are rewritten exactly as is_recluster
 * rewrites them.  from_pred of the reference (a file layout it no longer writes) has no counterpart.
 *
 * The keys of a frame are found first and ranked to `capacity` histogram slots of 1 KiB.  A frame with more keys than
 * that is never truncated: the call then changes NO frame's labels, flags or triples, and d_key_count reports the
 * frame's TRUE count (> capacity), which is how the caller learns of it (the call itself is asynchronous); the
 * per-key and per-stixel outputs are unspecified then.
 *
 * Zero-initialise before setting fields.  All device arrays are on the current device.
 *   d_sections, n_images, realcols, max_sections, rows, cols   as in is_render_args; n_images <= 65535,
 *                       rows * ceil(cols / 8), rows * (cols / realcols) and n_images * ceil(realcols / 4) fit 31 bits
 *   d_gt_instance       [n_images][rows][cols] int32, as is_assign_instances_gt takes it (4-byte aligned)
 *   d_disparity_u8      [n_images][rows][cols] uint8: what cv2.imread(path, IMREAD_GRAYSCALE) returns (:1074-1075)
 *                       (with cols % 8 == 0, a 16-byte aligned d_gt_instance and an 8-byte aligned d_disparity_u8 the
 *                       images are read with vector loads)
 *   instances           host [n_images], read before the call returns: every frame needs d_indices, d_centerofmass,
 *                       d_core_candidates, d_instances_per_class and d_labels; d_packed is optional
 *   eps, min_pts, size_filter   the clustering parameters; eps finite, min_pts >= 1
 *   capacity            histogram slots per frame, in [1, IS_INSTANCE_DISPARITY_KEYS]
 *   d_scratch           16-byte aligned, scratch_bytes >= is_instance_disparity_scratch_bytes(n_images, realcols,
 *                       max_sections, capacity); its contents mean nothing between calls
 *   d_stixel_median     optional, [n_images][realcols][max_sections] float: step 2, every slot written
 *   d_key_count         optional, [n_images] int32: the distinct keys of every frame
 *   d_key_median        optional, [n_images][IS_INSTANCE_DISPARITY_KEYS] uint16: step 1 in half units, 0 for a key
 *                       that is absent or has no non-zero disparity */
#define IS_INSTANCE_DISPARITY_KEYS 8000
typedef struct is_instance_disparity_args {
    const is_section* d_sections;
    const int32_t* d_gt_instance;
    const uint8_t* d_disparity_u8;
    int n_images, rows, cols, realcols, max_sections;
    const is_instance_buffers* instances;
    float eps;
    int min_pts, size_filter, capacity;
    void* d_scratch;
    size_t scratch_bytes;
    float* d_stixel_median;
    int32_t* d_key_count;
    uint16_t* d_key_median;
} is_instance_disparity_args;

/* Bytes of d_scratch for a call of that shape (0 for a shape or capacity the call refuses). */
size_t is_instance_disparity_scratch_bytes(int n_images, int realcols, int max_sections, int capacity);
/* The labels of n_images frames on `stream`, asynchronously and stream-ordered: one memset and six kinds of launch
 * (one clustering launch per 32 frames), no allocation, copy or synchronisation.  IS_EINVAL, with the reason in
 * is_last_error() and before any device call, for a null argument, a capacity outside its range, an eps that is not
 * finite, min_pts < 1, and for the shape, alignment and scratch constraints above. */
int is_cluster_instance_disparity(const is_instance_disparity_args* args, void* stream);

/* ---- f11: ground-truth offset targets and CNN offset channels (is_k_gt_targets.hip) ---------------------------------
 * Replaces the producer of the third "what if" row of the reference's instance evaluation, the CNN's two offset
 * channels taken from the ground truth (--usegtoffsets: tools/run_cityscapes.py:228,255-256 ->
 * tools/CNN_training/inference.py:388-396), which is also the producer of its training's regression targets
 * (tools/CNN_training/datasets/cityscapes.py:114-167 on images mode-downsampled by 8, datasets/transforms.py:49-70).
 * Per frame, with Hs = rows / 8 and Ws = cols / 8; rows and cols must be multiples of 8 (the reference's filter
 * raises on anything else):
 *   1. mode-downsample (modefilter_np, transforms.py:59-70): cell (y, x) takes the most frequent value of the block
 *      [8y, 8y + 8) x [8x, 8x + 8); ties go to the SMALLEST value (np.bincount(..).argmax()).  Negative int32 values
 *      are outside the reference's domain (bincount raises); here they are compared as signed values like any other.
 *   2. keys: a cell whose downsampled id is > 1000 has a key, the id itself (1000 has none, 1001 has one).  There is
 *      no class filter, as the reference has none: caravan and trailer ids and instanceTrainIds values work alike.
 *   3. offsets (_instance_offsets, cityscapes.py:146-167): per key, n = its cells, sy and sx = the INTEGER sums of
 *      their cell row and column indices; for each of its cells, in fp32 without contraction and with IEEE division
 *      (not a reciprocal: sum * (1 / n) differs from the reference, also after the conversion of step 5),
 *          off_y = (float)sy / (float)n - (float)y,    off_x = (float)sx / (float)n - (float)x;
 *      every other cell is (0, 0).  The reference sums in fp32, which is exact while a key's sums stay below 2^24 --
 *      always at Hs * Ws * max(Hs, Ws) < 2^24, e.g. 128 x 256 cells; beyond that the 64-bit integer sum rounded once
 *      is the definition.  The sums cannot wrap.
 *   4. disparity plane (_instance_offsets_disparity, :114-144), with the raw uint16 disparity image: mode-downsample
 *      it, q = v / 256 (integer); per key the LOWER median (torch.median) of its non-zero q, 0 where it has none, in
 *      every cell of the key; 0 in cells without a key.
 *   5. as prediction (inference.py:393-396 followed by FlipAndPad, wrappers.py:35-61): into d_segmentation
 *      [n_images][Ws][21][P2S] int32, for cell (y, x):
 *          seg[f][x][19][Hs-1-y] = (int32)(8.0f * off_y),    seg[f][x][20][Hs-1-y] = (int32)(8.0f * off_x)
 *      (truncation toward zero); rows Hs .. P2S-1 of both channels are written 0 and the 19 class channels are not
 *      touched: is_flip_and_pad of a CNN output whose last two channels were replaced by step 3, in the order (y, x)
 *      of the DP's channels 19 and 20 (StixelsKernels.cu:393-405).
 * The reference's own as_prediction assignment only fits its full-resolution models, the shapes do not match for the
 * downsampled ones it ships configs for; the 1/8-resolution semantics here are those of its training pipeline, the
 * only ones its DRNDS* models were ever given.
 *
 * With a disparity image the keys of a frame are numbered to `capacity` histograms of 1 KiB.  A frame with more keys
 * than that is never truncated: the call then writes NO output of any frame (targets, ids, segmentation) and
 * d_key_count reports the frame's TRUE count (> capacity), which is how the caller learns of it.
 *
 * Zero-initialise before setting fields.  All device arrays are on the current device.
 *   d_gt_instance       [n_images][rows][cols] int32, 4-byte aligned (16-byte aligned: vector loads); any value
 *   d_disparity_u16     optional, [n_images][rows][cols] uint16, 2-byte aligned (16-byte aligned: vector loads)
 *   n_images, rows, cols   n_images in [1, 65535]; rows, cols multiples of 8, >= 8; Hs * Ws <= 2^28
 *   d_targets, target_planes   optional, [n_images][target_planes][Hs][Ws] float: planes (off_y, off_x) with 2,
 *                       (disparity, off_y, off_x) with 3, which needs d_disparity_u16; target_planes is 0 without
 *   d_ids8              optional, [n_images][Hs][Ws] int32: step 1 of d_gt_instance
 *   d_segmentation, rows_power2_segmentation, channels   optional: step 5; P2S a power of two > Hs, channels == 21
 *                       (both 0 without d_segmentation).  At least one of the three outputs is required.
 *   capacity            histograms per frame, in [1, min(Hs * Ws, IS_GT_TARGETS_MAX_CAPACITY)]; 0 selects
 *                       min(256, Hs * Ws).  Without d_disparity_u16 it only has to be in range.
 *   d_scratch           16-byte aligned, scratch_bytes >= is_gt_targets_scratch_bytes(n_images, rows, cols,
 *                       with_disparity, capacity); its contents mean nothing between calls
 *   d_key_count         optional, [n_images] int32: the distinct keys of every frame, written also on overflow */
#define IS_GT_TARGETS_CHANNELS 21
#define IS_GT_TARGETS_MAX_CAPACITY 8192
#define IS_DTYPE_UINT8 0
#define IS_DTYPE_UINT16 1
#define IS_DTYPE_INT32 2
typedef struct is_gt_targets_args {
    const int32_t* d_gt_instance;
    const uint16_t* d_disparity_u16;
    int n_images, rows, cols;
    float* d_targets;
    int target_planes;
    int32_t* d_ids8;
    int32_t* d_segmentation;
    int rows_power2_segmentation, channels;
    int capacity;
    void* d_scratch;
    size_t scratch_bytes;
    int32_t* d_key_count;
} is_gt_targets_args;

/* Step 1 alone for n_images images [rows][cols] of dtype IS_DTYPE_* (instance ids, raw disparity, semantic gt):
 * d_dst [n_images][rows / 8][cols / 8] of the same type.  d_src and d_dst aligned to their element (a 16-byte aligned
 * d_src takes vector loads); rows and cols multiples of 8.  One launch on `stream`. */
int is_mode_downsample(const void* d_src, int dtype, int n_images, int rows, int cols, void* d_dst, void* stream);
/* Bytes of d_scratch for a call of that shape (0 for a shape or capacity the call refuses); capacity 0 as above. */
size_t is_gt_targets_scratch_bytes(int n_images, int rows, int cols, int with_disparity, int capacity);
/* The outputs of n_images frames on `stream`, asynchronously and stream-ordered: one memset and three launches
 * (six with a disparity image), no allocation, copy or synchronisation.  Integer atomics only: the same bytes on
 * every run.  IS_EINVAL, with the reason in is_last_error() and before any device call, for null or inconsistent
 * outputs, 3 planes without a disparity image, shapes that are not multiples of 8, a P2S that is not a power of two
 * > Hs, channels != 21, misaligned or undersized scratch and a capacity out of range. */
int is_gt_instance_targets(const is_gt_targets_args* args, void* stream);

/* ---- f12: the offset and disparity training losses of a batch, with their gradient (is_k_offset_loss.hip) ----------
 * The two "SL" regression losses the reference's DRN models were trained with (tools/CNN_training/losses.py:
 * OffsetLossSL :127-175, DisparityOffsetLossSL :24-125; used at train.py:127, 279, 322, 719-727), on the tensors f11
 * leaves on the device: the network's 2 or 3 regression channels at 1/8 resolution, the instance ids mode-downsampled
 * by 8 and the raw disparity mode-downsampled by 8.  One asynchronous call gives the loss, its four parts and
 * d loss / d prediction.  The definition is the reference's code evaluated in binary64 on the fp32 inputs (the
 * weights included, which arrive here as floats); the outputs are rounded to fp32 once, at the store.  Per frame:
 *
 *   Inputs.  P [planes][Hs][Ws] fp32: (off_y, off_x) with 2 planes, (disp, off_y, off_x) with 3 (the plane order of
 *   f11's targets).  ids [Hs][Ws] int32.  With 3 planes d8 [Hs][Ws] uint16 and q = d8 >> 8.  Cell (y, x) has the
 *   position (y, x) in image order: pos_y = off_y + y, pos_x = off_x + x.
 *   Keys.  Every id > 1000 is a key (1000 is none, 1001 is one; no class filter).  Per key k over its n cells:
 *   g = (sum y / n, sum x / n); m = the per-axis mean of pos; md = the mean of disp; med = the LOWER median
 *   (torch.median) of its non-zero q, which a key without a non-zero q does not have.
 *   Stuff.  A cell with id < 11 (negative ids included) or id == 255; there are s of them.  Every other cell
 *   (ids 11 .. 1000 without 255) contributes nothing and has the gradient 0.
 *   Terms.
 *     offset_mean          sum_k sum_cells (|pos_y - g_y| + |pos_x - g_x|) / n / 2  +  sum_stuff (|off_y| + |off_x|) / s / 2
 *     offset_variance      abs_variance == 0: sum_k (var_y + var_x) / 2, the population variance (0 for n == 1)
 *                          abs_variance != 0: sum_{k: n > 2} sum_cells (|pos_y - m_y| + |pos_x - m_x|) / n / 2
 *     disparity_variance   (3 planes) abs_variance == 0: sum_k var(disp);  else sum_{k: n > 2} sum_cells |disp - md| / n
 *     disparity_mean       (3 planes) sum_{k with a med} sum_cells |disp - med| / n  +  sum_stuff |disp| / s
 *                          (n counts ALL cells of the key)
 *     loss = w_offset_mean * offset_mean + w_offset_variance * offset_variance + w_disparity_mean * disparity_mean
 *            + w_disparity_variance * disparity_variance, each term summed over the frames first and NOT divided by
 *            the batch size.  With 2 planes the two disparity terms are 0 and are left out of the loss.
 *     A frame without stuff has NaN in offset_mean (and disparity_mean): the reference computes 0 / 0 there, and so
 *     does this; the frame's gradient stays finite.
 *   Gradient.  torch's, with d|v|/dv = sign(v) and sign(0) = 0; each line times its weight, the lines added:
 *     keyed, offset axes   offset_mean: sign(pos - g) / (2n)
 *                          offset_variance: (pos - m) / n;  abs form, n > 2: (sign(pos - m) - sum_j sign(pos_j - m) / n) / (2n)
 *                          (the reference does not detach the predicted mean)
 *     keyed, disparity     disparity_mean: sign(disp - med) / n where the key has a med
 *                          disparity_variance: 2 (disp - md) / n;  abs form, n > 2: (sign(disp - md) - sum_j sign(disp_j - md) / n) / n
 *     stuff                sign(off) / (2s) and sign(disp) / s
 *     A weight of 0 removes its lines from the gradient; the term itself is still reported.
 *   A non-finite prediction in a contributing cell makes the affected terms of ITS frame non-finite; the terms and
 *   gradients of the other frames are those of the clean batch.
 *
 * Every sum over predictions is binary64 and combined in an order the input alone decides (no floating-point
 * atomics; integer atomics for the key table and the q histograms): the same bytes on every run, the same bytes for a
 * frame alone and inside a batch, and the frames' terms and gradients follow a permutation of the frames.
 *
 * A frame's keys are ranked into `capacity` rows.  A frame with more keys than that is never truncated: d_loss and
 * d_terms become NaN, d_grad is left unwritten and d_key_count reports the TRUE counts.
 *
 * Zero-initialise before setting fields.  All device arrays are on the current device; floats and int32 4-byte
 * aligned, d_disparity8_u16 2-byte aligned.
 *   d_prediction, prediction_image_stride   frame f starts at d_prediction + f * stride (elements), its planes are
 *                       contiguous [planes][rows8][cols8]; stride >= planes * rows8 * cols8 (the last channels of a
 *                       wider tensor need no copy)
 *   d_ids8              [n_images][rows8][cols8] int32
 *   d_disparity8_u16    [n_images][rows8][cols8] uint16 with 3 planes, null with 2
 *   n_images, planes, rows8, cols8   n_images in [1, 65535]; planes 2 or 3; rows8 = Hs, cols8 = Ws >= 1; Hs * Ws <= 2^28
 *   w_*, abs_variance   the weights and the reference's abs_variance switch
 *   d_loss              [5] float: loss, offset_mean, offset_variance, disparity_mean, disparity_variance (batch sums)
 *   d_terms             optional, [n_images][4] float: the frames' four terms
 *   d_grad, grad_image_stride   optional: d loss / d prediction laid out as the prediction with its own stride
 *                       (>= planes * rows8 * cols8); all planes of every frame are written, zeros included
 *   capacity            rows per frame, in [1, min(Hs * Ws, IS_GT_TARGETS_MAX_CAPACITY)]; 0 selects min(256, Hs * Ws)
 *   d_scratch           16-byte aligned, scratch_bytes >= is_offset_loss_scratch_bytes(n_images, planes, rows8, cols8,
 *                       capacity); its contents mean nothing between calls
 *   d_key_count         optional, [n_images] int32: the distinct keys of every frame, written also on overflow */
typedef struct is_offset_loss_args {
    const float* d_prediction;
    long long prediction_image_stride;
    const int32_t* d_ids8;
    const uint16_t* d_disparity8_u16;
    int n_images, planes, rows8, cols8;
    float w_offset_mean, w_offset_variance, w_disparity_mean, w_disparity_variance;
    int abs_variance;
    float* d_loss;
    float* d_terms;
    float* d_grad;
    long long grad_image_stride;
    int capacity;
    void* d_scratch;
    size_t scratch_bytes;
    int32_t* d_key_count;
} is_offset_loss_args;

/* Bytes of d_scratch for a call of that shape (0 for a shape or capacity the call refuses); capacity 0 as above. */
size_t is_offset_loss_scratch_bytes(int n_images, int planes, int rows8, int cols8, int capacity);
/* The losses of n_images frames on `stream`, asynchronously and stream-ordered: one memset and eight launches (nine
 * with d_grad), no allocation, copy or synchronisation.  IS_EINVAL, with the reason in is_last_error() and before any
 * device call, for a null required pointer, planes outside {2, 3}, a disparity pointer that does not go with planes,
 * non-positive shapes, Hs * Ws > 2^28, a stride below planes * Hs * Ws, misaligned pointers, misaligned or undersized
 * scratch, a capacity out of range and n_images outside [1, 65535]. */
int is_offset_loss(const is_offset_loss_args* args, void* stream);

/* ---- f13: the CNN's segmentation head of a batch, straight to the DP's input (is_k_head.hip) ------------------------
 * The last layers of the reference's models and its export wrapper in one launch with fixed numerics:
 * DRNDSDoubleSeg.forward (tools/CNN_training/models/DRNDownsampled.py:97-102: `seg`, a 1x1 convolution from the
 * backbone's K features to n_classes + n_regression channels, -LogSoftmax over the classes, the concatenation),
 * DRNDSOffsetDisparity.forward (:128-137: the same with a disparity channel, clamped to [0, 128] in eval mode),
 * FlipAndPad (models/wrappers.py:35-61) and the sign that inference.py:374 gives the other models' output.
 * Backbone features in, the DP's d_segmentation out, optionally the float network output that is_flip_and_pad takes.
 *
 *   Logits.   z[c] = fmaf(w[c][K-1], x[K-1], ... fmaf(w[c][0], x[0], bias[c]) ...): one fp32 chain in increasing k,
 *             started from the bias; no split-K, no partial sums combined afterwards.  (On the device the f32-input
 *             MFMA, issued in k order onto one accumulator: bit for bit that chain.)
 *   Classes.  c < n_classes: y[c] = (m + log(sum_j exp(z[j] - m))) - z[c], m = max_j z[j] over the n_classes logits,
 *             evaluated in binary64 and rounded to fp32 once: -log_softmax.
 *   Regression channels pass through unchanged; channel clamp_channel is clamped to [clamp_lo, clamp_hi].
 *   d_cnn_out holds those values; d_segmentation holds (int32)(8.0f * value), rows flipped, zero in every pad row:
 *             byte for byte what is_flip_and_pad makes of d_cnn_out.  Every element of both is written (no memset).
 *   The same bytes on every run; a frame's result does not depend on its position in the batch or on n_images.
 *   Non-finite logits give unspecified values, never a write outside the outputs.
 *
 * Zero-initialise, then set the fields (clamp_channel = -1 for no clamp).  All arrays on the current device.
 *   d_features          [n_images][K][rows8][cols8], contiguous NCHW, of dtype IS_HEAD_F32 / _F16 / _BF16, aligned to
 *                       its element; halves are widened to fp32 at the load, which is exact
 *   d_weight, d_bias    [channels_out][K] and [channels_out] fp32 (seg.weight without its two unit dimensions)
 *   n_images, K, rows8, cols8   n_images in [1, 65535]; K >= 8 and a multiple of 8; rows8, cols8 >= 1
 *   n_classes, n_regression     n_classes >= 1, n_regression >= 0, channels_out = their sum <= IS_HEAD_MAX_CHANNELS
 *   rows_power2_segmentation    a power of two >= rows8 + 1
 *   clamp_channel, clamp_lo, clamp_hi   -1, or a regression channel (>= n_classes) and clamp_lo <= clamp_hi
 *   d_cnn_out           optional, [n_images][channels_out][rows8][cols8] fp32
 *   d_segmentation      optional, [n_images][cols8][channels_out][rows_power2_segmentation] int32; at least one of
 *                       the two outputs is given
 *   reserved            0 */
#define IS_HEAD_MAX_CHANNELS 32
#define IS_HEAD_F32 0
#define IS_HEAD_F16 1
#define IS_HEAD_BF16 2
typedef struct is_segmentation_head_args {
    const void* d_features;
    int dtype;
    int n_images, K, rows8, cols8;
    const float* d_weight;
    const float* d_bias;
    int n_classes, n_regression;
    int rows_power2_segmentation;
    int clamp_channel;
    float clamp_lo, clamp_hi;
    float* d_cnn_out;
    int32_t* d_segmentation;
    int reserved[4]; /* 0 */
} is_segmentation_head_args;

/* One launch on `stream`, asynchronous and stream-ordered; no allocation, copy or synchronisation.  IS_EINVAL, with
 * the reason in is_last_error() and before the device is touched, for null args, a null input, both outputs null, an
 * unknown dtype, a shape, channel split, K or rows_power2_segmentation outside the ranges above, a clamp_channel that
 * is no regression channel, misaligned pointers and a non-zero reserved field. */
int is_segmentation_head(const is_segmentation_head_args* args, void* stream);

/* ---- f14: the backward pass of the segmentation head and the semantic NLL loss (is_k_head_backward.hip, is_k_nll.hip)
 * What training through f13's head needs (the reference trains every model as closs + rloss, tools/CNN_training/
 * train.py:698-732, closs = nn.NLLLoss(reduction='mean', ignore_index=255) on the class channels, train.py:281-282,
 * 325-326; optim_seg_parameters, DRNDownsampled.py:139-143, is head-only fine-tuning): the gradient of f13's float
 * output with respect to the features, the weight and the bias, and the classification loss with its gradient.  The
 * rule is f13's: every summation order is fixed by the input's shape alone, no floating-point atomics, the same bytes
 * on every run.
 *
 * Notation.  CH = n_classes + n_regression <= IS_HEAD_MAX_CHANNELS, P = rows8 * cols8, pixel p = row * cols8 + col.
 * y is f13's d_cnn_out [n][CH][rows8][cols8] fp32, saved from the forward and not recomputed; gy is the upstream
 * gradient with respect to y, in the same layout with its own image stride.
 *
 *   Logit gradient dz [n][CH][P] fp32.  Class channel j < n_classes: S = sum_{c < n_classes} (double)gy[c] in
 *             increasing c, dz[j] = (float)(exp(-(double)y[j]) * S - (double)gy[j]), in binary64 and rounded once
 *             (from y[c] = lse - z[c]).  Regression channel: dz[c] = gy[c], bit for bit.  No clamp: the reference
 *             clamps only in eval mode (DRNDownsampled.py:133-134).
 *   d_grad_features [n][K][rows8][cols8] in the dtype of the features: dX[k][p] is the fp32 chain
 *             acc = fmaf(w[c][k], dz[c][p], acc) for c = 0 .. CH-1, started from +0.0f; rounded once (to nearest
 *             even) for fp16 / bf16 features.  Every element is written.  A frame's dX does not depend on n_images
 *             or on its position in the batch.
 *   d_grad_weight [CH][K], d_grad_bias [CH] fp32.  The contraction over all n * P pixels is split, and the split is
 *             part of the contract: chunk j of image i covers p in [j T, min((j + 1) T, P)), T =
 *             IS_HEAD_BACKWARD_CHUNK for every shape.  part[i][j][c][k] is the fp32 chain
 *             acc = fmaf(dz[c][p], x[k][p], acc) in increasing p from +0.0f;
 *             dW[c][k] = (float) sum (double)part[i][j][c][k], i outer and j inner, both increasing, rounded once.
 *             db[c] is the same with x = 1, i.e. acc = acc + dz[c][p] in fp32.  Halves are widened at the load.
 *   d_grad_logits [n][CH][rows8][cols8] fp32 receives dz (so that the two contractions can be checked bit for bit on
 *             the device's own dz).
 *   No floating-point atomics, nothing depends on the grid, the same bytes on every run and for every choice of the
 *   optional outputs.  Non-finite inputs give unspecified values, never a write outside the outputs; no address
 *   depends on a value.
 *
 * Zero-initialise, then set the fields.  All arrays on the current device.
 *   d_features, dtype, n_images, K, rows8, cols8, d_weight, n_classes, n_regression   as in f13, the same ranges, and
 *                       rows8 * cols8 <= 2^28
 *   d_cnn_out           y, [n_images][CH][rows8][cols8] fp32, contiguous
 *   d_grad_out, grad_image_stride   gy: frame f starts at d_grad_out + f * stride (elements), its planes are
 *                       contiguous [CH][rows8][cols8]; stride >= CH * P
 *   d_grad_features, d_grad_weight, d_grad_bias, d_grad_logits   optional, at least one of them is given
 *   d_scratch           16-byte aligned, scratch_bytes >= is_segmentation_head_backward_scratch_bytes(...); its
 *                       contents mean nothing between calls
 *   reserved            0 */
#define IS_HEAD_BACKWARD_CHUNK 2048
typedef struct is_segmentation_head_backward_args {
    const void* d_features;
    int dtype;
    int n_images, K, rows8, cols8;
    const float* d_weight;
    int n_classes, n_regression;
    const float* d_cnn_out;
    const float* d_grad_out;
    long long grad_image_stride;
    void* d_grad_features;
    float* d_grad_weight;
    float* d_grad_bias;
    float* d_grad_logits;
    void* d_scratch;
    size_t scratch_bytes;
    int reserved[4]; /* 0 */
} is_segmentation_head_backward_args;

/* Bytes of d_scratch for a call of that shape, channels = n_classes + n_regression (0 for a shape the call refuses). */
size_t is_segmentation_head_backward_scratch_bytes(int n_images, int K, int rows8, int cols8, int channels);
/* One to three launches on `stream` (dz and dX; the chunk partials; their reduction), asynchronous and
 * stream-ordered; no allocation, copy or synchronisation.  IS_EINVAL, with the reason in is_last_error() and before
 * the device is touched, for null args, a null required pointer, all four outputs null, an unknown dtype, a shape,
 * channel split or K outside the ranges above, a stride below CH * P, misaligned pointers, scratch that is too small
 * or misaligned and a non-zero reserved field. */
int is_segmentation_head_backward(const is_segmentation_head_backward_args* args, void* stream);

/* The classification loss of the reference's training, nn.NLLLoss(reduction='mean', ignore_index) on f13's class
 * planes (which hold -log p), with its gradient:
 *   d_cnn_out, cnn_image_stride   frame f starts at d_cnn_out + f * stride (elements); its first n_classes planes
 *                       [rows8][cols8] are read; stride >= n_classes * P
 *   d_target, target_dtype   [n_images][rows8][cols8], IS_DTYPE_UINT8 or IS_DTYPE_INT32 (what is_mode_downsample
 *                       writes for the semantic ground truth)
 *   n_images, rows8, cols8, n_classes   n_images in [1, 65535], rows8, cols8 >= 1, P <= 2^28, n_images * P < 2^31,
 *                       n_classes in [1, IS_HEAD_MAX_CHANNELS]
 *   d_loss              [1] float: (float)(sum_valid (double)y[t_p](p) / V); the sum is binary64, combined in an order
 *                       the shape alone decides; V = 0 gives NaN, as torch does
 *   d_valid_count       [1] int32: V, the pixels whose target is a class
 *   d_bad_count         [1] int32: targets outside [0, n_classes) that are not ignore_index; they count as ignored
 *   d_grad, grad_image_stride   optional: [c == t_p] * (float)(1.0 / V) in all n_classes planes of every frame, zeros
 *                       included, laid out as d_cnn_out with its own stride (>= n_classes * P); all zero with V = 0.
 *                       With f12's d_grad on the regression planes this assembles one gy without memset or copy.
 *   d_scratch           16-byte aligned, scratch_bytes >= is_semantic_nll_scratch_bytes(n_images, rows8, cols8)
 *   reserved            0
 * Two launches (three with d_grad), asynchronous and stream-ordered, no allocation, copy, synchronisation or atomics.
 * IS_EINVAL as above. */
typedef struct is_semantic_nll_args {
    const float* d_cnn_out;
    long long cnn_image_stride;
    const void* d_target;
    int target_dtype;
    int ignore_index;
    int n_images, rows8, cols8, n_classes;
    float* d_loss;
    int32_t* d_valid_count;
    int32_t* d_bad_count;
    float* d_grad;
    long long grad_image_stride;
    void* d_scratch;
    size_t scratch_bytes;
    int reserved[4]; /* 0 */
} is_semantic_nll_args;

size_t is_semantic_nll_scratch_bytes(int n_images, int rows8, int cols8);
int is_semantic_nll(const is_semantic_nll_args* args, void* stream);

/* ---- f15: the CNN's own label maps of a batch at full resolution, scored on the device (is_k_cnn_labels.hip) -------
 * The reference's evaluation prints the IoU of the CNN alone beside the stixels' (tools/run_cityscapes.py:353-365,
 * 551: run_cityscapesevaluation_CNN on the labelImg.png files under probs/) and its training selects models by it
 * (tools/CNN_training/train.py:559-605, validation_snapshot).  The label image behind that row is the per-pixel
 * arg-min of the network output brought to full resolution: by interpolate(scale_factor=8, mode='nearest') for the
 * downsampled models (tools/CNN_training/inference.py:286-292, 373-381), by the fixed bilinear `up` layer for the
 * full-resolution ones (models/DRNSeg.py:35-44, 64-79: ConvTranspose2d(C, C, 16, stride=8, padding=4, groups=C)
 * with fill_up_weights).  Here in one launch from f13's d_cnn_out: no upsampled plane is ever written, the label
 * image is written once and the ground truth is read once for f5's confusion table.
 *
 *   Inputs.   The planes are costs, as the DP reads them: v[c] = d_cnn_out[i][c][y][x] for c < n_classes (f13's
 *             -log_softmax).  Planes n_classes .. channels-1 are not read.
 *   Arg-min.  The class of a value vector is the first strict minimum in increasing c:
 *             best = 0; for c = 1 ..: if (v[c] < v[best]) best = c.  A NaN never replaces the current best; all-NaN
 *             gives 0.
 *   d_class8  the class of the cell's own n_classes values, in both modes.
 *   IS_CNN_UP_NEAREST   pixel (Y, X) with X < 8 * cols8 takes the class of cell (Y / 8, X / 8).
 *   IS_CNN_UP_DECONV    the 1-D weight of tap k in 0..15 is W[k] = (2 * min(k, 15 - k) + 1) / 16.0f.  Output
 *             coordinate o receives input i in {(o + 4) / 8 - 1, (o + 4) / 8} intersected with [0, n), with
 *             k = o + 4 - 8 i; the 2-D weight is W[ky] * W[kx], exact in fp32.  The upsampled value of class c is the
 *             fp32 chain acc = fmaf(w, v, acc) from +0.0f over the taps in the order (iy low, ix low), (iy low,
 *             ix high), (iy high, ix low), (iy high, ix high).  A tap outside the plane is SKIPPED, not multiplied by
 *             zero: +inf in a border cell stays +inf and never becomes NaN.  The pixel's class is the arg-min rule
 *             on those values.  (The reference applies `up` to the logits and takes the arg-max of their log-softmax.
 *             By linearity the upsampled cost planes differ from the upsampled logits by a per-pixel constant and
 *             the sign, so the two agree in exact arithmetic; in fp32 they may differ at near-ties.  The contract is
 *             the chain on the cost planes.)
 *   d_label   class_to_label[class]; a class outside the table gives 0; pixels with X >= 8 * cols8 are 0.  Every
 *             element is written.
 *   d_confusion   f5's convention, what evaluation.cityscapes_iou takes: [n_labels][n_labels] uint64, ADDED to:
 *             conf[gt][pred] += 1 for every pixel with X < 8 * cols8, gt < n_labels and pred < n_labels, summed over
 *             the batch.  Integer atomics only: the same table on every run.
 *   A frame's outputs do not depend on its position in the batch or on n_images; no address depends on a value.
 *
 * Zero-initialise, then set the fields.  All device arrays on the current device.
 *   d_cnn_out           [n_images][channels][rows8][cols8] fp32, 4-byte aligned
 *   n_images, channels, n_classes, rows8, cols8   n_images in [1, 65535]; n_classes in [1, IS_HEAD_MAX_CHANNELS];
 *                       channels >= n_classes; rows8, cols8 >= 1; channels * rows8 * cols8 < 2^31
 *   mode                IS_CNN_UP_NEAREST or IS_CNN_UP_DECONV
 *   rows, cols          the image: rows == 8 * rows8, cols >= 8 * cols8, rows * cols < 2^31
 *   h_class_to_label    host [n_classes]; NULL: Cityscapes trainId -> labelId, as f5 (19 entries)
 *   d_class8            optional [n_images][rows8][cols8] uint8
 *   d_label             optional [n_images][rows][cols] uint8
 *   d_gt_label, d_confusion   both or neither: gt [n_images][rows][cols] uint8; the table 8-byte aligned, n_labels in
 *                       [1, IS_RENDER_MAX_LABELS]
 *   reserved            0 */
#define IS_CNN_UP_NEAREST 0   /* inference.py:286-292 */
#define IS_CNN_UP_DECONV  1   /* DRNSeg.py: the fixed 16 / 8 / 4 transposed convolution */
typedef struct is_cnn_label_args {
    const float* d_cnn_out;
    int n_images, channels, n_classes, rows8, cols8;
    int mode;
    int rows, cols;
    const uint8_t* h_class_to_label;
    uint8_t* d_class8;
    uint8_t* d_label;
    const uint8_t* d_gt_label;
    int n_labels;
    unsigned long long* d_confusion;
    int reserved[4]; /* 0 */
} is_cnn_label_args;

/* One launch on `stream`, asynchronous and stream-ordered; no allocation, copy or synchronisation.  IS_EINVAL, with
 * the reason in is_last_error() and before the device is touched, for null args, a null d_cnn_out, no output at all,
 * only one of d_gt_label and d_confusion, an unknown mode, rows != 8 * rows8 or cols < 8 * cols8, a shape, n_classes,
 * channels or n_labels outside the ranges above, n_images outside [1, 65535], rows * cols or channels * rows8 * cols8
 * of 2^31 or more, a misaligned d_cnn_out or d_confusion and a non-zero reserved field. */
int is_cnn_label_maps(const is_cnn_label_args* args, void* stream);

/* ---- f16: the full-resolution semantic NLL through the fixed `up` layer, with its gradient (is_k_nll_up.hip) -------
 * The training counterpart of f15's IS_CNN_UP_DECONV.  The reference's full-resolution models (tools/CNN_training/
 * models/DRNSeg.py:46-225: DRNSeg, DRNDoubleSeg, DRNOffsetDisparity) compute seg -> up -> LogSoftmax and are trained
 * with nn.NLLLoss(reduction='mean', ignore_index=255) on full-resolution ground truth (train.py:69-232).  Here on
 * f13's cost planes y = -log_softmax(z): `up` is linear with the same weights for every class, so -up(y) differs from
 * up(z) by one constant per pixel (also at the border, where taps are skipped) and log_softmax(-up(y)) ==
 * log_softmax(up(z)) in exact arithmetic.  The gradient with respect to y sums to zero over the classes of a cell, so
 * is_segmentation_head_backward turns it into the reference's dL/dz.  No upsampled plane is ever stored.
 *
 *   u_c       of pixel (Y, X), X < 8 * cols8: f15's IS_CNN_UP_DECONV fmaf chain on the cost planes of class c, bit for
 *             bit the value is_cnn_label_maps compares.
 *   Per pixel, in fp32, each operation rounded once: m = min_c u_c; S = sum_c expf(m - u_c) in increasing c from
 *             +0.0f; K = m - logf(S); L_pix = u_t - K; p_c = expf(K - u_c); the residual r_c = [c == t] - p_c.
 *             expf and logf are the device library's (the OpenCL C bounds they are built to: 3 ulp each).
 *   Valid     a pixel with X < 8 * cols8 whose target t is in [0, n_classes) and is not ignore_index.  V is their
 *             number; d_bad_count the pixels with X < 8 * cols8 whose target is neither a class nor ignore_index
 *             (they count as ignored, as in f14).  Pixels with X >= 8 * cols8 take no part.
 *   d_loss    (float)(sum_valid (double)L_pix / V): a binary64 sum, combined in an order the shape alone decides (per
 *             frame first, then over the frames in increasing order, so that a batch of equal frames has the loss of
 *             one); V = 0 gives NaN, as torch does.
 *   d_grad    grad[i][c][cy][cx] = inv_V * sum W[ky] W[kx] r_c over the valid pixels of the cell's 16 x 16 footprint
 *             that lie inside the image (W as in f15), inv_V = (float)(1.0 / V) applied as one final fp32 multiply;
 *             all zero with V = 0.  The fp32 order of the sum, fixed by the shape: the footprint is the four 8 x 8
 *             blocks Y = 8a-4 .. 8a+3, X = 8b-4 .. 8b+3 for a in {cy, cy+1}, b in {cx, cx+1}.  In a block, a row's
 *             h = fmaf(W[kx], r, h) in increasing X from +0.0f, then G = fmaf(W[ky], h, G) in increasing Y from +0.0f
 *             (rows outside the image skipped, pixels that do not count have r = +0.0f); the cell is
 *             ((G(cy, cx) + G(cy, cx+1)) + G(cy+1, cx)) + G(cy+1, cx+1).  All n_classes planes of every frame are
 *             written, zeros included, laid out as d_cnn_out with its own stride: with f12's d_grad on the regression
 *             planes this assembles one gy without memset or copy.
 *   No floating-point atomics; nothing depends on the grid, on a frame's position in the batch or on n_images other
 *   than through inv_V; the same bytes on every run, and the same loss and counts with and without d_grad.
 *   Non-finite planes give unspecified values, never a write outside the outputs; no address depends on a plane's
 *   value.
 *
 * Zero-initialise, then set the fields.  All arrays on the current device.
 *   d_cnn_out, cnn_image_stride   frame f starts at d_cnn_out + f * stride (elements); its first n_classes planes
 *                       [rows8][cols8] are read; stride >= n_classes * rows8 * cols8
 *   d_target            [n_images][rows][cols] uint8 class ids (trainIds)
 *   n_images, rows8, cols8, n_classes, rows, cols   n_images in [1, 65535]; rows8, cols8 >= 1; n_classes in
 *                       [1, IS_HEAD_MAX_CHANNELS]; rows == 8 * rows8, cols >= 8 * cols8; rows * cols < 2^31 and
 *                       n_classes * rows8 * cols8 < 2^31 (the offsets inside a frame)
 *   mode                IS_CNN_UP_DECONV; IS_CNN_UP_NEAREST is refused: the loss at 1/8 resolution is is_semantic_nll
 *   d_loss              [1] float
 *   d_valid_count, d_bad_count   [1] int64 each, 8-byte aligned: n_images * rows * cols < 2^47 always fits
 *   d_grad, grad_image_stride   optional, stride >= n_classes * rows8 * cols8; without it the call is the validation
 *                       loss and computes no residual
 *   d_scratch           16-byte aligned, scratch_bytes >= is_semantic_nll_up_scratch_bytes(...); its contents mean
 *                       nothing between calls
 *   reserved            0 */
typedef struct is_semantic_nll_up_args {
    const float* d_cnn_out;
    long long cnn_image_stride;
    const uint8_t* d_target;
    int ignore_index;
    int n_images, rows8, cols8, n_classes;
    int mode;
    int rows, cols;
    float* d_loss;
    int64_t* d_valid_count;
    int64_t* d_bad_count;
    float* d_grad;
    long long grad_image_stride;
    void* d_scratch;
    size_t scratch_bytes;
    int reserved[4]; /* 0 */
} is_semantic_nll_up_args;

/* Bytes of d_scratch for a call of that shape (0 for a shape the call refuses). */
size_t is_semantic_nll_up_scratch_bytes(int n_images, int rows8, int cols8, int n_classes);
/* Two launches (three with d_grad: the tiles, the reduction of their records, the scaling by inv_V), asynchronous and
 * stream-ordered; no allocation, copy or synchronisation.  IS_EINVAL, with the reason in is_last_error() and before
 * the device is touched, for null args, a null d_cnn_out or d_target, a null d_loss, d_valid_count or d_bad_count, an
 * unknown mode or IS_CNN_UP_NEAREST, rows != 8 * rows8 or cols < 8 * cols8, a shape or n_classes outside the ranges
 * above, n_images outside [1, 65535], a stride below n_classes * rows8 * cols8, misaligned pointers, scratch that is
 * null, too small or misaligned and a non-zero reserved field. */
int is_semantic_nll_up(const is_semantic_nll_up_args* args, void* stream);

/* ---- f17: the backbone's tail, a dilated 3x3 convolution + BatchNorm + ReLU of a batch (is_k_conv3x3.hip) ------------
 * The two layers in front of f13's head, the same in every model of the reference: layer7 and layer8 of the DRN
 * (tools/CNN_training/models/drn.py:181-185, built by _make_conv_layers, drn.py:223-233: Conv2d(C, C, 3, padding =
 * dilation, dilation = 2 and 1, bias = False) + BatchNorm2d + ReLU), which the reference runs in half precision
 * (amp "O1", inference.py:278).  In one launch per layer on the half-precision MFMA, with BatchNorm folded to one
 * scale and shift per channel, so that layer7 -> layer8 -> is_segmentation_head is three launches of this library
 * with nothing in between.  fp32 features are out of scope (the f32-input MFMA has 1/16 of the rate): convert first.
 *
 *   Operands.    The half values: the features as given, the weights as is_conv3x3_pack_weights rounded them (round to
 *                nearest even).  A product of two of them is exact in fp32.
 *   Summation.   a[n][co][y][x] = sum over the 9 taps and all channels_in of
 *                w[co][ci][ky][kx] * x[n][ci][y + (ky - 1) dilation][x + (kx - 1) dilation]; a tap outside the image
 *                contributes nothing (zero padding = dilation, stride 1).  Accumulated in fp32 MFMA accumulators by
 *                v_mfma_f32_32x32x16_f16 / _bf16, one accumulator chain per output element: no split over workgroups,
 *                no atomics, no partial sums combined afterwards.
 *   Order.       The order of the MFMA instructions along (tap, channel) is fixed by the shape alone: 16-channel chunks
 *                in increasing order, the taps 3 ky + kx of a chunk in increasing order.  The summation INSIDE one
 *                instruction (16 products) is the hardware's and is not specified.  This entry point is therefore
 *                pinned by a derived error bound plus inputs whose arithmetic is exact in every order, NOT by a C loop
 *                that gives its bits -- a weaker contract than f13's fmaf chain, and said so here on purpose.
 *   Epilogue.    v = fmaf(scale[co], a, shift[co]) in fp32, then max(v, 0) when relu is set.  With out_dtype =
 *                IS_HEAD_F32 that value is stored, with a half out_dtype its round-to-nearest-even conversion.
 *   Determinism. The same bytes on every run; a frame's result does not depend on its position in the batch or on
 *                n_images.
 *   Non-finite values give unspecified values, never an access outside the buffers; no address depends on a value.
 *
 * Weights: d_weight is conv.weight, [channels_out][channels_in][3][3] fp32.  is_conv3x3_pack_weights rounds each to the
 * half dtype (round to nearest even) and writes them in an opaque layout of the kernel's choosing that holds exactly
 * those values, is_conv3x3_packed_bytes(...) bytes at a 16-byte aligned d_packed: one small launch, once per model.
 *
 * Zero-initialise, then set the fields.  All arrays on the current device.
 *   d_features, dtype   [n_images][channels_in][rows8][cols8], contiguous NCHW, IS_HEAD_F16 or IS_HEAD_BF16, aligned to
 *                       the element; no row alignment is asked for (cols8 = 7 is legal)
 *   n_images            in [1, 65535];  rows8, cols8 in [1, 32767]
 *   channels_in         a multiple of 16 in [16, 2048];  channels_out a multiple of 32 in [32, 2048]
 *   dilation            in [1, 8]
 *   d_packed            from is_conv3x3_pack_weights with the same channels and dtype, 16-byte aligned
 *   d_scale, d_shift    [channels_out] fp32: the folded BatchNorm (scale = gamma / sqrt(var + eps), shift = beta -
 *                       mean * scale)
 *   relu                0 or 1
 *   d_out, out_dtype    [n_images][channels_out][rows8][cols8] of the input's dtype or IS_HEAD_F32, aligned to its
 *                       element; every element is written; its bytes must not overlap the features' (the halo makes
 *                       an in-place call wrong)
 *   reserved            0 */
typedef struct is_conv3x3_args {
    const void* d_features;
    int dtype;
    int n_images, channels_in, channels_out, rows8, cols8, dilation;
    const void* d_packed;
    const float* d_scale;
    const float* d_shift;
    int relu;
    void* d_out;
    int out_dtype;
    int reserved[4]; /* 0 */
} is_conv3x3_args;

/* Bytes of d_packed (0 for arguments outside the ranges above). */
size_t is_conv3x3_packed_bytes(int channels_out, int channels_in, int dtype);
/* One launch on `stream`, asynchronous.  IS_EINVAL before the device is touched for null pointers, channels or a dtype
 * outside the ranges above and misaligned pointers. */
int is_conv3x3_pack_weights(const float* d_weight, int channels_out, int channels_in, int dtype, void* d_packed,
                            void* stream);
/* One launch on `stream`, asynchronous and stream-ordered; no allocation, copy or synchronisation.  IS_EINVAL, with
 * the reason in is_last_error() and before the device is touched, for null args or pointers, dtype IS_HEAD_F32 or
 * unknown, an out_dtype that is neither the input's nor IS_HEAD_F32, any argument outside the ranges above, relu
 * outside {0, 1}, a misaligned d_packed (or another pointer off its element), output and feature byte ranges that
 * overlap and a non-zero reserved field. */
int is_conv3x3_bn_relu(const is_conv3x3_args* args, void* stream);

/* ---- f18: the backbone's residual blocks, convolution + BatchNorm (+ residual) (+ ReLU) of a batch (is_k_conv3x3.hip) -
 * layer5 and layer6 of the DRN behind every shipped config (drn_d_22; tools/CNN_training/models/drn.py:168-172): each
 * two BasicBlocks (drn.py:54-87) built by _make_layer(..., new_level = False) (drn.py:199-221), 128 -> 256 -> 512
 * channels, dilations (2, 2) and (4, 4), stride 1, at 1/8 resolution in the NCHW half layout f17 reads.  A block is
 *     out = relu(bn1(conv1(x)));  out = bn2(conv2(out));  out += downsample(x) or x;  out = relu(out)
 * with downsample = Conv2d(1x1, bias = False) + BatchNorm2d in the first block of a layer.  f17's entry point cannot
 * express the residual operand between the BatchNorm and the ReLU, nor the 1x1 convolution; is_conv3x3_args cannot grow.
 * This entry point is f17's with both, so that layer5 -> layer6 -> layer7 -> layer8 -> head is thirteen launches of this
 * library with nothing in between; is_conv3x3_bn_relu is this call with kernel = 3 and no residual, the same launch
 * and the same bytes, and is_conv_pack_weights(kernel = 3) writes the bytes of is_conv3x3_pack_weights.
 *
 *   Operands.    The half values: the features and the residual as given, the weights as is_conv_pack_weights rounded
 *                them (round to nearest even).  A product of two of them is exact in fp32, and so is a widened residual.
 *   Summation.   kernel = 3: f17's, over the 9 taps and all channels_in.  kernel = 1: a[n][co][y][x] = sum over all
 *                channels_in of w[co][ci] * x[n][ci][y][x].  Accumulated in fp32 MFMA accumulators by
 *                v_mfma_f32_32x32x16_f16 / _bf16, one accumulator chain per output element: no split over workgroups,
 *                no atomics, no partial sums combined afterwards.
 *   Order.       The MFMA instructions of an element follow each other in increasing 16-channel chunk and, inside a
 *                chunk, in increasing tap 3 ky + kx: fixed by the shape alone.  The summation INSIDE one instruction
 *                (16 products) is the hardware's and is not specified: as f17, this entry point is pinned by a derived
 *                error bound plus inputs whose arithmetic is exact in every order, not by a C loop.
 *   Epilogue.    In fp32, three steps:
 *                    v = fmaf(scale[co], a, shift[co])
 *                    v = v + (float)residual[n][co][y][x]      when d_residual is given (the widening is exact)
 *                    v = max(v, 0)                             when relu is set
 *                then the store: that value with out_dtype = IS_HEAD_F32, its round-to-nearest-even conversion with a
 *                half out_dtype.  With a residual these are two fp32 roundings (the fmaf, the addition) before the
 *                single final rounding to the half dtype.  The reference adds the residual on HALF tensors under amp
 *                (bn2's half output, `out += residual`, drn.py:84: one more rounding to half in between); this
 *                contract adds it in fp32 before the single final rounding, and says so on purpose.
 *   Determinism. The same bytes on every run; a frame's result does not depend on its position in the batch or on
 *                n_images.
 *   Non-finite values give unspecified values, never an access outside the buffers; no address depends on a value.
 *
 * Weights: d_weight is conv.weight, [channels_out][channels_in][kernel][kernel] fp32; is_conv_pack_weights rounds each
 * to the half dtype (round to nearest even) into is_conv_packed_bytes(...) bytes at a 16-byte aligned d_packed, in an
 * opaque layout that holds exactly those values.
 *
 * Zero-initialise, then set the fields.  All arrays on the current device.  Fields as in is_conv3x3_args, and
 *   kernel              3 or 1 (the convolution is kernel x kernel, padding = dilation * (kernel - 1) / 2, stride 1)
 *   dilation            kernel 3: in [1, 8];  kernel 1: must be 1
 *   d_packed            from is_conv_pack_weights with the same channels, kernel and dtype, 16-byte aligned
 *   d_residual          NULL, or [n_images][channels_out][rows8][cols8] of `dtype` (the OUTPUT's shape), aligned to its
 *                       element.  Exactly its n_images * channels_out * rows8 * cols8 elements are read.  It may be
 *                       the features themselves (channels_in = channels_out: a block without downsample); its bytes
 *                       must not overlap the output's
 *   d_out               its bytes must overlap neither the features' nor the residual's */
typedef struct is_conv_bn_args {
    const void* d_features;
    int dtype; /* IS_HEAD_F16 | IS_HEAD_BF16 */
    int n_images, channels_in, channels_out, rows8, cols8;
    int kernel;   /* 3 or 1 */
    int dilation; /* kernel 3: [1, 8];  kernel 1: must be 1 */
    const void* d_packed;
    const float* d_scale;
    const float* d_shift;
    const void* d_residual; /* NULL, or [n][channels_out][rows8][cols8] of `dtype` */
    int relu;
    void* d_out;
    int out_dtype;
    int reserved[4]; /* 0 */
} is_conv_bn_args;

/* Bytes of d_packed: channels_out * channels_in * kernel * kernel * 2 (0 for arguments outside the ranges). */
size_t is_conv_packed_bytes(int channels_out, int channels_in, int kernel, int dtype);
/* One launch on `stream`, asynchronous.  IS_EINVAL before the device is touched for null pointers, channels, a kernel
 * or a dtype outside the ranges above and misaligned pointers. */
int is_conv_pack_weights(const float* d_weight, int channels_out, int channels_in, int kernel, int dtype,
                         void* d_packed, void* stream);
/* One launch on `stream`, asynchronous and stream-ordered; no allocation, copy or synchronisation.  IS_EINVAL, with
 * the reason in is_last_error() and before the device is touched, for everything is_conv3x3_bn_relu refuses, a kernel
 * outside {1, 3}, dilation != 1 with kernel 1, a residual off its element alignment and residual bytes that overlap
 * the output's. */
int is_conv_bn(const is_conv_bn_args* args, void* stream);

/* ---- f19: the backbone's downsampling layers, the same launch with stride 1 or 2 (is_k_conv3x3.hip) -------------------
 * layer2, layer3 and layer4 of drn_d_22 (tools/CNN_training/models/drn.py:161-167; layers [1, 1, 2, 2, 2, 2, 1, 1],
 * channels (16, 32, 64, 128, 256, 512, 512, 512)): layer2 is Conv2d(16, 32, 3, stride = 2, padding = 1, bias = False) +
 * BatchNorm2d + ReLU (_make_conv_layers, drn.py:223-233), layer3 and layer4 are two BasicBlocks each (_make_layer(...,
 * new_level = True), drn.py:199-221, dilation (1, 1)), 32 -> 64 -> 128 channels, whose first block has stride 2 in its
 * conv1 (3x3) and in its downsample (1x1).  Every other convolution of the three layers is a stride-1, dilation-1 3x3
 * that is_conv_bn runs.  is_conv_bn_args cannot grow and its reserved fields stay refused, so this entry point stands
 * beside it as f18's stands beside f17's: is_conv_bn is this call with stride = 1, the same launch and the same bytes,
 * and layer2 -> ... -> layer8 -> head is 24 launches of this library with nothing in between, from layer1's output at
 * full resolution to the DP's input.  These layers are not at 1/8 resolution: the extents are rows_in, cols_in.
 *
 *   Output.      stride 1: rows_in x cols_in.  stride 2: rows_out = (rows_in + 1) / 2 by cols_out = (cols_in + 1) / 2 in
 *                integer division -- torch's floor((H + 2 p - d (k - 1) - 1) / 2) + 1, which is ceil(H / 2) both for
 *                (k = 3, p = 1, d = 1) and for (k = 1, p = 0).  The output extents are derived, not fields.
 *   Summation.   stride 2, kernel 3: a[n][co][y][x] = sum over the 9 taps and all channels_in of
 *                w[co][ci][ky][kx] * x[n][ci][2 y + ky - 1][2 x + kx - 1];  kernel 1: of w[co][ci] * x[n][ci][2 y][2 x].
 *                A tap outside the image contributes nothing: with an even extent the bottom / right padding is never
 *                read, with an odd extent it is.  stride 2 means dilation 1 (the reference has no other).
 *   Operands, order, epilogue, determinism and non-finite values: is_conv_bn's, unchanged.  One accumulator chain per
 *                output element in increasing 16-channel chunk, then increasing tap 3 ky + kx; no atomics; the three
 *                fp32 steps v = fmaf(scale[co], a, shift[co]), v + (float)residual[n][co][y][x], max(v, 0), then the
 *                store.  Every output index, every predicate and the residual use the OUTPUT's extents.
 *   Loads.       No address outside the features' n_images * channels_in * rows_in * cols_in elements is loaded from.
 *
 * Weights: the packed layout does not depend on the stride; is_conv_pack_weights and is_conv_packed_bytes serve.
 *
 * Zero-initialise, then set the fields.  Fields as in is_conv_bn_args, and
 *   d_features          [n_images][channels_in][rows_in][cols_in];  rows_in, cols_in in [1, 32767]
 *   stride              1 or 2;  2 needs dilation 1
 *   d_residual          NULL, or [n_images][channels_out][rows_out][cols_out] of `dtype` (the OUTPUT's shape).  With
 *                       stride 2 it cannot be the features (the shapes differ)
 *   d_out               [n_images][channels_out][rows_out][cols_out]; its bytes must overlap neither the features' nor
 *                       the residual's, each taken at its own size
 *   reserved            0 */
typedef struct is_conv_bn_stride_args {
    const void* d_features;
    int dtype; /* IS_HEAD_F16 | IS_HEAD_BF16 */
    int n_images, channels_in, channels_out, rows_in, cols_in;
    int kernel;   /* 3 or 1 */
    int stride;   /* 1 or 2 */
    int dilation; /* kernel 3: [1, 8], 1 with stride 2;  kernel 1: must be 1 */
    const void* d_packed;
    const float* d_scale;
    const float* d_shift;
    const void* d_residual; /* NULL, or [n][channels_out][rows_out][cols_out] of `dtype` */
    int relu;
    void* d_out;
    int out_dtype;
    int reserved[4]; /* 0 */
} is_conv_bn_stride_args;

/* One launch on `stream`, asynchronous and stream-ordered; no allocation, copy or synchronisation.  IS_EINVAL, with
 * the reason in is_last_error() and before the device is touched, for everything is_conv_bn refuses (the extents are
 * named rows_in and cols_in), a stride outside {1, 2}, stride 2 with dilation != 1, stride 2 with d_residual ==
 * d_features, and, last, a non-zero reserved field. */
int is_conv_bn_stride(const is_conv_bn_stride_args* args, void* stream);

/* ---- f20: the backbone's stem, image bytes to layer1's output of a batch in one launch (is_k_stem.hip) -------------
 * layer0 and layer1 of drn_d_22 (tools/CNN_training/models/drn.py:154-159: Conv2d(3, 16, 7, stride 1, padding 3, bias =
 * False) + BatchNorm2d + ReLU;  drn.py:161-162, _make_conv_layers with layers[0] == 1: Conv2d(16, 16, 3, padding 1,
 * bias = False) + BatchNorm2d + ReLU) and, in front of them, what the reference does to the camera image: ToTensor,
 * Normalize and the cast to half (inference.py:109-110, :278).  is_conv_bn_stride cannot take these layers (3 and 16
 * channels are below its tiles and it has no 7x7), and the two belong in one launch: layer0's output stays in LDS, so
 * the compulsory traffic is 3 + 32 bytes per pixel instead of (3 + 32) + (32 + 32).  is_stem -> 23 x is_conv_bn_stride ->
 * is_segmentation_head is 25 launches of this library with nothing in between: image bytes in, the DP's input out.
 *
 *     x[n][c][y][x]  = lut[c][ image[n][y][x][c] ]                       c in 0..2
 *     mid            = half( relu( bn0( conv7x7(x), pad 3 ) ) )          3 -> 16 channels
 *     out            = half( relu( bn1( conv3x3(mid), pad 1 ) ) )        16 -> 16 channels
 *
 *   Input.       d_image is uint8 [n_images][rows][cols][3]: interleaved, contiguous, as a decoder delivers it.  d_lut
 *                is [3][256] of the half `dtype`.  The operand of layer0 at channel c is lut[c][byte], and that is the
 *                whole definition of the normalisation: the launch gives the table's bits.  Byte position c pairs with
 *                input channel c of layer0's weight; a BGR caller permutes the table's rows and the weight's input
 *                channels.
 *   Padding 0.   A tap of layer0 outside the image contributes nothing: zero padding of the NORMALISED value.  It is
 *                not lut[c][0], and it cannot be folded into weights or shift.
 *   mid.         a0 = sum over 3 x 7 x 7 of w0[co][ci][ky][kx] * x[n][ci][y + ky - 3][x + kx - 3], accumulated in fp32
 *                by v_mfma_f32_16x16x32_{f16,bf16} on ONE accumulator chain per element, in an order fixed by the shape
 *                alone (one instruction per ky, in increasing ky); zero-filled k slots are exact zeros; the order inside
 *                one instruction is the hardware's, as in f17.  Then v = fmaf(scale0[co], a0, shift0[co]), max(v, 0),
 *                rounded to `dtype` to nearest even.  layer1's operands are exactly these half values.
 *   Padding 1.   A mid pixel outside the image is ZERO: not relu(shift0) and not a convolution evaluated past the edge.
 *   out.         a1 = sum over 16 x 3 x 3 of w1[co][ci][ky][kx] * mid[n][ci][y + ky - 1][x + kx - 1] with the same
 *                rules (increasing tap 3 ky + kx, 16 channels a tap); then fmaf(scale1[co], a1, shift1[co]), max(., 0),
 *                rounded to nearest even to `dtype`.  d_out is [n][16][rows][cols] NCHW contiguous, what
 *                is_conv_bn_stride reads for layer2.  Every element is written.
 *   d_mid.       NULL, or [n][16][rows][cols] of `dtype`: every element of mid is also stored.  d_out has the same bytes
 *                whether or not d_mid is given; with d_mid == NULL mid never reaches global memory.  A mid halo pixel
 *                computed by two workgroups has the same bits in both, because the order is the same.
 *   Determinism. The same bytes on every run; a frame's result does not depend on its position in the batch or on
 *                n_images; no atomics.
 *   Safety.      No address outside the image's n_images * rows * cols * 3 bytes is loaded from.  Non-finite table
 *                entries give unspecified values and never a wild access: no address depends on a value other than the
 *                table index, which is a byte.
 *   Ranges.      n_images in [1, 65535]; rows, cols in [1, 32767] with no multiple-of-anything requirement.  The
 *                channels are 3 -> 16 -> 16, kernel 7 / pad 3 and kernel 3 / pad 1, stride 1, dilation 1: not fields.
 *
 * Weights: d_w0 is layer0's conv.weight [16][3][7][7], d_w1 layer1's [16][16][3][3], fp32.  is_stem_pack_weights
 * rounds each to the half dtype (round to nearest even) into one opaque blob that holds exactly those values (and
 * zeros), is_stem_packed_bytes(dtype) bytes at a 16-byte aligned d_packed: one small launch, once per model.
 *
 * Zero-initialise, then set the fields.  All arrays on the current device.
 *   d_image             [n_images][rows][cols][3] uint8
 *   d_lut               [3][256] of `dtype`, aligned to its element
 *   d_packed            from is_stem_pack_weights with the same dtype, 16-byte aligned
 *   d_scale0 .. d_shift1   [16] fp32 each: the folded BatchNorms of layer0 and layer1
 *   d_mid               NULL, or [n_images][16][rows][cols] of `dtype`
 *   d_out               [n_images][16][rows][cols] of `dtype`; its bytes must overlap neither d_mid's nor the image's,
 *                       and d_mid's not the image's, each taken at its own size
 *   reserved            0 */
typedef struct is_stem_args {
    const void* d_image;
    int n_images, rows, cols;
    const void* d_lut;
    int dtype; /* IS_HEAD_F16 | IS_HEAD_BF16 */
    const void* d_packed;
    const float* d_scale0;
    const float* d_shift0;
    const float* d_scale1;
    const float* d_shift1;
    void* d_mid; /* NULL, or [n][16][rows][cols] of `dtype` */
    void* d_out;
    int reserved[4]; /* 0 */
} is_stem_args;

/* The bytes of the packed weights; 0 for a dtype that is neither IS_HEAD_F16 nor IS_HEAD_BF16. */
size_t is_stem_packed_bytes(int dtype);
/* One small launch on `stream`.  IS_EINVAL for null pointers, a dtype as above, d_w0 / d_w1 off 4-byte alignment or
 * d_packed off 16-byte alignment. */
int is_stem_pack_weights(const float* d_w0 /*[16][3][7][7]*/, const float* d_w1 /*[16][16][3][3]*/, int dtype,
                         void* d_packed, void* stream);
/* One launch on `stream`, asynchronous and stream-ordered; no allocation, copy or synchronisation.  IS_EINVAL, with
 * the reason in is_last_error() and before the device is touched, for null args or required pointers (all but d_mid);
 * a dtype that is IS_HEAD_F32 or unknown; n_images, rows or cols out of range; d_packed off 16-byte alignment, d_lut,
 * d_mid or d_out off their element, a fold off 4 bytes; d_out overlapping d_mid, or either of them overlapping the
 * image, each taken at its own byte size; and, last, a non-zero reserved field. */
int is_stem(const is_stem_args* args, void* stream);

/* ---- f21: the backward pass of convolution + BatchNorm (+ residual) (+ ReLU), stride 1 (is_k_conv_backward.hip) ------
 * What fine-tuning more than the head needs (the reference trains the whole base, optim_parameters yields
 * base.parameters() in all but one configuration of tools/CNN_training/train.py): the gradients of is_conv_bn's output
 * with respect to the features, the fp32 master weight, the folded scale and shift and the residual operand, by f14's
 * rules: every summation order fixed by the shape alone, no floating-point atomics, the same bytes on every run.
 *
 * BatchNorm is FROZEN at its running statistics: (scale, shift) are the folded pair the forward takes, and this is
 * the backward of exactly that forward.  The reference's train.py:947 runs NN.train() with batch statistics; that is a
 * different forward and is not built.  Stride 1 only (layer5 .. layer8; stride 2 and the stem are not built).
 *
 * Forward (f18), a = conv(x, w):  v = fmaf(scale[co], a, shift[co]);  v += residual;  v = max(v, 0) with relu.
 * P = rows8 * cols8, taps = kernel * kernel, d = dilation, w_half = the half rounding of w that is_conv_pack_weights makes.
 *
 *   gh [n][co][P], half dtype.  gh = round_half(dY) where relu is 0 or the STORED out is > 0, else +0 (round to nearest
 *             even; a dY of the half dtype passes through).  An output that rounded to 0 is inactive, as torch's ReLU
 *             backward.  gh is the gradient with respect to the residual operand (d_grad_pre), and the one operand
 *             every other gradient is computed from.  fp16 under- and overflow of gh is the caller's loss scaling.
 *   dshift[co] = (float) sum (double)gh[n][co][p], in binary64: a block of 256 threads takes 2048 consecutive p of one
 *             plane, a thread 8 of them in increasing p, then an LDS tree (t += t + s, s = 128 .. 1); one block per co
 *             adds the blocks' sums, n outer and block inner, as contiguous thread ranges and the same tree.
 *   dX [n][ci][P], half dtype or fp32: the stride-1 convolution of gh, same kernel, dilation and padding, with
 *             wT[ci][co][taps - 1 - tap] = round_half(scale[co] * w_half[co][ci][tap]) (the product in fp32, rounded
 *             once), run by is_conv_bn's own launch with the channels swapped, scale 1, shift 0, relu 0: f18's
 *             operands, order, bound and determinism word for word.  d_grad_features_add, dX's shape in the half
 *             dtype, is that launch's residual operand: added in fp32 before the single final rounding.  Needs
 *             channels_in % 32 == 0.  A frame's gh and dX do not depend on n_images or its position in the batch.
 *   G[co][ci][tap] = sum over n, y, x of gh[n][co][y][x] * x[n][ci][y + (ky - 1) d][x + (kx - 1) d]; a tap outside
 *             the image contributes nothing.  The contraction is split and the split is part of the contract: chunk
 *             (i, j) is image i, rows [j B, min((j + 1) B, rows8)), B = IS_CONV_BACKWARD_BAND for every shape.  Inside a
 *             chunk ONE fp32 MFMA accumulator per (co, ci, tap), fed by v_mfma_f32_32x32x16_{f16,bf16} in an order
 *             the shape fixes: 32-pixel segments of the rows in increasing column; in a segment the chunk's rows by
 *             residue class mod d (kernel 1: d = 1) and increasing inside a class; in a row the two 16-pixel steps in
 *             increasing column (the lanes past the row's end are zero); the operands are
 *             half values, their products exact in fp32; the summation of the 16 products inside one instruction is
 *             the hardware's.  As f17, pinned by a derived bound plus exact-arithmetic inputs, not by a C loop.
 *             Gsum = sum (double)part[i][j], i outer, j inner, both increasing.
 *   dW[co][ci][tap] = (float)((double)scale[co] * Gsum[co][ci][tap]), rounded once; conv.weight's layout; the gradient
 *             with respect to the fp32 master weight, straight through the half rounding.
 *   dscale[co] = (float) sum (double)w_half[co][ci][tap] * Gsum[co][ci][tap] in binary64, in increasing (ci, tap):
 *             contiguous ranges of 256 threads, then the LDS tree above.
 *   Every output is optional, at least one is asked for; leaving one out changes no byte of the others and skips the
 *   launches it alone needs.  Non-finite values give unspecified values, never an access outside the buffers; no
 *   address depends on a value.
 *
 * Zero-initialise, then set the fields.  All arrays on the current device.
 *   d_features, dtype, n_images, channels_in, channels_out, rows8, cols8, kernel, dilation   as in is_conv_bn_args
 *   d_weight            conv.weight [channels_out][channels_in][kernel][kernel] fp32 (NOT the packed weights)
 *   d_scale             [channels_out] fp32
 *   d_out, out_dtype    the forward's saved output [n][channels_out][rows8][cols8], `dtype` or IS_HEAD_F32; read with
 *                       relu = 1 only (it may be NULL with relu = 0)
 *   d_grad_out, grad_out_dtype, grad_image_stride   dY, `dtype` or IS_HEAD_F32: frame f starts at d_grad_out + f *
 *                       stride (elements), its planes contiguous [channels_out][rows8][cols8]; stride >= channels_out P
 *   d_grad_features, grad_features_dtype   dX, `dtype` or IS_HEAD_F32;  d_grad_features_add: NULL or `dtype`, with dX only
 *   d_grad_weight, d_grad_scale, d_grad_shift   fp32;  d_grad_pre: gh, `dtype`
 *   d_scratch           16-byte aligned, scratch_bytes >= is_conv_bn_backward_scratch_bytes(...); its contents mean
 *                       nothing between calls
 *   reserved            0 */
#ifndef IS_CONV_BACKWARD_BAND /* (an experiment build may define another; the product's value is this one) */
#define IS_CONV_BACKWARD_BAND 32
#endif
typedef struct is_conv_bn_backward_args {
    const void* d_features;
    int dtype; /* IS_HEAD_F16 | IS_HEAD_BF16 */
    int n_images, channels_in, channels_out, rows8, cols8;
    int kernel;   /* 3 or 1 */
    int dilation; /* kernel 3: [1, 8];  kernel 1: must be 1 */
    const float* d_weight;
    const float* d_scale;
    const void* d_out;
    int out_dtype;
    int relu;
    const void* d_grad_out;
    int grad_out_dtype;
    long long grad_image_stride;
    void* d_grad_features;
    int grad_features_dtype;
    const void* d_grad_features_add;
    float* d_grad_weight;
    float* d_grad_scale;
    float* d_grad_shift;
    void* d_grad_pre;
    void* d_scratch;
    size_t scratch_bytes;
    int reserved[4]; /* 0 */
} is_conv_bn_backward_args;

/* Bytes of d_scratch for a call of that shape (0 for a shape the call refuses): gh, the transposed pack, the dshift
 * block sums, Gsum in binary64 and n_images * ceil(rows8 / B) partials of channels_out * channels_in * taps fp32. */
size_t is_conv_bn_backward_scratch_bytes(int n_images, int channels_in, int channels_out, int rows8, int cols8, int kernel,
                                         int dtype);
/* Up to six launches on `stream` (gh and the dshift block sums; the transposed pack; dX by is_conv_bn's launch; the
 * chunk partials; their reduction; dscale and dshift per channel), fewer with outputs left out; asynchronous and
 * stream-ordered; no allocation, copy or synchronisation.  IS_EINVAL, with the reason in is_last_error() and before
 * the device is touched, for everything is_conv_bn refuses, no output asked for, d_grad_features with channels_in %
 * 32 != 0, d_grad_features_add without d_grad_features, a dtype of out, dY or dX that is neither `dtype` nor
 * IS_HEAD_F32, a stride below channels_out * P, misaligned pointers, output bytes that overlap an input's or another
 * output's, scratch that is too small or misaligned and, last, a non-zero reserved field.  There is no stride field:
 * a stride-2 layer cannot be expressed, and the Python layer refuses it with a message. */
int is_conv_bn_backward(const is_conv_bn_backward_args* args, void* stream);

/* ---- f22: the backward pass of is_conv_bn_stride, stride 1 or 2 (is_k_conv_backward.hip, is_k_conv_backward_stride.hip) --
 * The five stride-2 launches of drn_d_22 (layer2; conv1 and downsample of layer3[0] and layer4[0]) get their backward.
 * is_conv_bn_backward_args cannot grow and its reserved fields stay refused, so this entry point stands beside it as
 * is_conv_bn_stride stands beside is_conv_bn: with stride = 1 the call IS is_conv_bn_backward -- one checker, one
 * launcher, the same launches, bytes, scratch size and messages, the extents named rows_in / cols_in.
 *
 * At stride 2 (dilation 1; kernel 3 with padding 1 or kernel 1) rows_out = (rows_in + 1) / 2, cols_out = (cols_in + 1) / 2
 * are derived, P = rows_out * cols_out, and f21's rules hold word for word except:
 *
 *   gh, dshift  f21's, over the OUTPUT's P (the same launches).
 *   G[co][ci][tap] = sum over n, y, x of gh[n][co][y][x] * x[n][ci][2 y + ky - 1][2 x + kx - 1] (kernel 1: x[n][ci][2 y]
 *             [2 x]); a tap outside the image contributes nothing (with an even extent the bottom / right padding is
 *             never touched, with an odd one it is).  Chunk (i, j) is image i and OUTPUT rows [j B, min((j + 1) B,
 *             rows_out)), B = IS_CONV_BACKWARD_STRIDE_BAND for every shape; no column split.  Inside a chunk ONE fp32
 *             MFMA accumulator per (co, ci, tap), fed by v_mfma_f32_32x32x16_{f16,bf16}: 32-pixel segments of the
 *             OUTPUT rows in increasing column; in a segment the chunk's rows in increasing y; in a row the two
 *             16-pixel steps in increasing column (the lanes past the row's end are zero).  Gsum, dW and dscale: f21's
 *             binary64 reductions (the same launches).
 *   dX[n][ci][r][c] = sum over co and over the taps (ky, kx) with r + 1 - ky and c + 1 - kx both even and y = (r + 1 -
 *             ky) / 2 in [0, rows_out), x = (c + 1 - kx) / 2 in [0, cols_out), of wT[ci][co][tap] * gh[n][co][y][x], wT =
 *             round_half(scale[co] * w_half[co][ci][tap]) as in f21.  The four (row, column) parity classes of an
 *             element use 1, 2, 2 and 4 taps at kernel 3; at kernel 1 only (even, even) elements get a sum and every
 *             other element is exactly +0 (or the features_add value).  ONE fp32 MFMA accumulator chain per element,
 *             not split and not combined: increasing 16-channel chunk of channels_out and, inside a chunk, increasing
 *             tap 3 ky + kx among the element's class (v_mfma_f32_32x32x16, the 16 products of one instruction in the
 *             hardware's order).  d_grad_features_add is added in fp32 before the single final rounding.  Every
 *             element of dX is written.  Needs channels_in % 32 == 0: layer2 (16 channels in) gets dW, dscale and
 *             dshift only, its dX has no consumer until the stem has a backward.
 *
 * Fields as in is_conv_bn_backward_args, and
 *   rows_in, cols_in    the INPUT's extents: d_features, d_grad_features, d_grad_features_add are [n][channels_in][rows_in]
 *                       [cols_in]
 *   stride              1 or 2;  2 needs dilation 1
 *   d_out, d_grad_out, d_grad_pre   the OUTPUT's extents [n][channels_out][rows_out][cols_out]; grad_image_stride >=
 *                       channels_out * rows_out * cols_out
 *   reserved            0 */
#ifndef IS_CONV_BACKWARD_STRIDE_BAND /* (an experiment build may define another; the product's value is this one) */
#define IS_CONV_BACKWARD_STRIDE_BAND 8
#endif
typedef struct is_conv_bn_stride_backward_args {
    const void* d_features;
    int dtype; /* IS_HEAD_F16 | IS_HEAD_BF16 */
    int n_images, channels_in, channels_out, rows_in, cols_in;
    int kernel;   /* 3 or 1 */
    int stride;   /* 1 or 2 */
    int dilation; /* kernel 3: [1, 8], 1 with stride 2;  kernel 1: must be 1 */
    const float* d_weight;
    const float* d_scale;
    const void* d_out;
    int out_dtype;
    int relu;
    const void* d_grad_out;
    int grad_out_dtype;
    long long grad_image_stride;
    void* d_grad_features;
    int grad_features_dtype;
    const void* d_grad_features_add;
    float* d_grad_weight;
    float* d_grad_scale;
    float* d_grad_shift;
    void* d_grad_pre;
    void* d_scratch;
    size_t scratch_bytes;
    int reserved[4]; /* 0 */
} is_conv_bn_stride_backward_args;

/* Bytes of d_scratch for a call of that shape (0 for a shape the call refuses); with stride 1,
 * is_conv_bn_backward_scratch_bytes' value.  At stride 2 the sections have the OUTPUT's extents and n_images *
 * ceil(rows_out / IS_CONV_BACKWARD_STRIDE_BAND) partials. */
size_t is_conv_bn_stride_backward_scratch_bytes(int n_images, int channels_in, int channels_out, int rows_in, int cols_in,
                                                int kernel, int stride, int dtype);
/* is_conv_bn_backward's launches, with dX by k_conv_bwd_data_s2 and the partials by k_conv_bwd_weight_s2 at stride 2.
 * IS_EINVAL, with the reason in is_last_error() and before the device is touched, for everything is_conv_bn_backward
 * refuses (the extents are named rows_in and cols_in), a stride outside {1, 2}, stride 2 with dilation != 1 and, last, a
 * non-zero reserved field. */
int is_conv_bn_stride_backward(const is_conv_bn_stride_backward_args* args, void* stream);

/* ---- f23: the backward pass of the stem, layer0 and layer1 (is_k_stem_backward.hip) ----------------------------------
 * The backward of exactly is_stem's forward: BatchNorm folded and frozen, the operands the half values the forward
 * used, f21's rules (every summation order fixed by the shape alone, no floating-point atomics, the same bytes on every
 * run and for every choice of outputs, a frame's gh planes independent of n_images and of its position in the batch, no
 * address that depends on a value other than the table index, no load outside the image's bytes or the tensors'
 * extents; non-finite values give unspecified values, never a wild access).  With it every parameter of drn_d_22 has a
 * gradient on the device.  There is no gradient for the table or the image.
 *
 * w*_half = the half rounding is_stem_pack_weights makes; P = rows * cols.
 *
 *   g_out [n][16][rows][cols]   the gradient with respect to `out`, from exactly one of two sources:
 *             (a) d_grad_out (dY), `dtype` or IS_HEAD_F32, frame f at d_grad_out + f * grad_image_stride elements, as
 *             f21's;
 *             (b) d_grad_next, the masked gradient gh of the stride-2 3x3 layer that reads `out` (layer2's d_grad_pre of
 *             f22, [n][channels_next][(rows + 1) / 2][(cols + 1) / 2] of `dtype`), with that layer's master weight
 *             d_weight_next [channels_next][16][3][3] and folded scale d_scale_next: f22's stride-2 dX formula at kernel
 *             3 with 16 input channels, g_out[n][ci][r][c] = sum over co and over the taps (ky, kx) with r + 1 - ky and
 *             c + 1 - kx both even and y = (r + 1 - ky) / 2, x = (c + 1 - kx) / 2 inside gh, of wT[ci][co][tap] *
 *             gh[n][co][y][x], wT = round_half(scale_next[co] * w_next_half[co][ci][tap]); the parity classes use 1, 2,
 *             2 and 4 taps.  ONE fp32 MFMA accumulator chain per element (v_mfma_f32_16x16x32), in increasing 32-channel
 *             chunk of channels_next and, inside a chunk, increasing tap 3 ky + kx among the element's class; rounded
 *             once to `dtype`.  g_out is computed by a launch of its own into the scratch (the fusion
 *             into the next launch is not built; the bytes are the same).
 *   gh1 = round_half(g_out) where the STORED out > 0, else +0.
 *   dshift1[co] = (float) sum (double)gh1, in binary64: a workgroup of k_stem_bwd_data owns a tile of IS_STEM_BACKWARD_TILE_ROWS
 *             x IS_STEM_BACKWARD_TILE_COLS pixels of one frame; thread (row r, channel co) adds its row of the tile in
 *             increasing column, then the 16 rows in increasing r; one block per co adds the tiles' sums, image outer
 *             and tile inner (row-major), as contiguous thread ranges and f21's LDS tree (k_conv_bwd_channel).
 *   dMid [n][16][rows][cols] = the 3x3, padding-1 convolution of gh1 with wT1[ci][co][8 - tap] = round_half(scale1[co] *
 *             w1_half[co][ci][tap]) (the product in fp32, rounded once); a tap outside the image contributes nothing.
 *             ONE fp32 accumulator chain per element by v_mfma_f32_16x16x32_{f16,bf16}: five instructions in increasing
 *             k = 16 tap' + co, tap' = 8 - tap, the slots k >= 144 exact zeros on both operands; rounded once to `dtype`.
 *   gh0 = dMid where the STORED mid > 0, else +0.
 *   dshift0[co] = (float) sum (double)gh0: a lane of k_stem_bwd_data adds its four pixels of a 16-pixel group in increasing
 *             column and its groups in increasing order (row-major in the tile, every fourth group to a wave); the 16
 *             lanes of a channel are added in increasing (wave, lane >> 4); then as dshift1.
 *   G1[co][ci][tap] = sum gh1[n][co][y][x] * mid[n][ci][y + ky - 1][x + kx - 1]
 *   G0[co][c][ky][kx] = sum gh0[n][co][y][x] * lut[c][image[n][y + ky - 3][x + kx - 3][c]]; a tap outside the image
 *             contributes nothing (zero padding of the normalised value, not lut[c][0]).
 *             The contraction over pixels is split and the split is part of the contract: chunk (i, j, k) is image i,
 *             rows [j B, (j + 1) B), columns [k S, (k + 1) S), B = IS_STEM_BACKWARD_BAND and S =
 *             IS_STEM_BACKWARD_SEGMENT for every shape.  Inside a chunk ONE fp32 MFMA accumulator per (co, ci, tap), fed
 *             by v_mfma_f32_16x16x32_{f16,bf16} with pixels on K: the chunk's rows in increasing y, in a row the S / 32
 *             steps of 32 pixels in increasing column (the slots past the row's end or outside the image are exact
 *             zeros).  Gsum = the binary64 sum of the partials, i outer, then j, then k, increasing.
 *   dW = (float)((double)scale[co] * Gsum), conv.weight's layout;  dscale[co] = (float) sum (double)w_half * Gsum in
 *             increasing (ci, tap): f21's reductions (k_conv_bwd_reduce, k_conv_bwd_channel), their instantiations.
 *   Every output is optional, at least one is asked for; leaving one out changes no byte of the others.  The launch
 *   of the partials and the reductions run only when an output needs them.
 *
 * Zero-initialise, then set the fields.  All arrays on the current device.
 *   d_image, n_images, rows, cols, d_lut, dtype   as in is_stem_args
 *   d_w0, d_w1          the fp32 master weights [16][3][7][7] and [16][16][3][3] (NOT the pack)
 *   d_scale0, d_scale1  [16] fp32
 *   d_mid, d_out        the forward's saved tensors [n][16][rows][cols] of `dtype` (is_stem with d_mid given)
 *   d_grad_out, grad_out_dtype, grad_image_stride   dY; stride >= 16 P
 *   d_grad_next, channels_next, d_weight_next, d_scale_next   source (b); channels_next % 32 == 0, in [32, 128]
 *   d_grad_weight0 .. d_grad_shift1   fp32: [16][3][7][7], [16], [16], [16][16][3][3], [16], [16]
 *   d_grad_pre1, d_grad_pre0   gh1 and gh0, [n][16][rows][cols] of `dtype`; without them they live in the scratch
 *   d_scratch           16-byte aligned, scratch_bytes >= is_stem_backward_scratch_bytes(...)
 *   reserved            0 */
#ifndef IS_STEM_BACKWARD_BAND /* (an experiment build may define another; the product's value is this one) */
#define IS_STEM_BACKWARD_BAND 64
#endif
#define IS_STEM_BACKWARD_SEGMENT 64
#define IS_STEM_BACKWARD_TILE_ROWS 16
#define IS_STEM_BACKWARD_TILE_COLS 64
typedef struct is_stem_backward_args {
    const void* d_image;
    int n_images, rows, cols;
    const void* d_lut;
    int dtype; /* IS_HEAD_F16 | IS_HEAD_BF16 */
    const float* d_w0;
    const float* d_w1;
    const float* d_scale0;
    const float* d_scale1;
    const void* d_mid;
    const void* d_out;
    const void* d_grad_out;
    int grad_out_dtype;
    long long grad_image_stride;
    const void* d_grad_next; /* source (b), or NULL */
    int channels_next;       /* 0 with source (a) */
    const float* d_weight_next;
    const float* d_scale_next;
    float* d_grad_weight0;
    float* d_grad_scale0;
    float* d_grad_shift0;
    float* d_grad_weight1;
    float* d_grad_scale1;
    float* d_grad_shift1;
    void* d_grad_pre1;
    void* d_grad_pre0;
    void* d_scratch;
    size_t scratch_bytes;
    int reserved[4]; /* 0 */
} is_stem_backward_args;

/* Bytes of d_scratch for a call of that shape (0 for a shape the call refuses): gh1 and gh0, the transposed pack, the
 * dshift tile sums, Gsum in binary64 and the chunks' partials; with channels_next != 0 (source (b)) also g_out and that
 * layer's pack.  channels_next = 0 is source (a). */
size_t is_stem_backward_scratch_bytes(int n_images, int rows, int cols, int channels_next, int dtype);
/* Up to nine launches on `stream` (with source (b) the next layer's pack and g_out; the transposed pack; gh1, dMid, gh0
 * and the dshift tile sums; the chunk partials of G1 and G0; their two reductions; dscale and dshift per channel,
 * twice), fewer with outputs left out; asynchronous and stream-ordered; no allocation, copy or synchronisation.
 * IS_EINVAL, with the reason in is_last_error() and before the device is touched, for null args or required pointers;
 * everything is_stem refuses for the fields they share; both or neither gradient source; channels_next out of range; a
 * grad_out_dtype that is neither `dtype` nor IS_HEAD_F32; a stride below 16 * rows * cols; misaligned pointers; output bytes that overlap
 * an input's or another output's; a scratch that is too small or misaligned; no output asked for; and, last, a non-zero
 * reserved field. */
int is_stem_backward(const is_stem_backward_args* args, void* stream);
/* IS_STEM_BACKWARD_BAND, IS_STEM_BACKWARD_SEGMENT, IS_STEM_BACKWARD_TILE_ROWS and IS_STEM_BACKWARD_TILE_COLS of the
 * library as it was built (which = 0 .. 3; -1 for another). */
int is_stem_backward_constant(int which);

/* ---- f9: per-instance objects and their contours (is_k_objects.hip) ------------------------------------------------
 * What the reference's consumers reduce on the host from the per-stixel output: the top-down view
 * (tools/visualization/clustering_visualization.py:563-792: per instance and column the closest stixel, connected
 * into a contour, and a mean disparity of the instance) and the per-instance masks (draw_instance_masks :118-142,
 * the union of the rectangles of all stixels of one instance).  Here as a keyed reduction on the device, per frame
 * over the key (class, label), with w = cols / realcols (integer division) as in f5 / f6 / f8.
 *
 * Members.  A section in front of its column's terminator, whatever its type, is a member of instance (c, l) of its
 * frame when its semantic_class is c in 11..18 and its d_section_instance value is l with 0 <= l < 1000 -- exactly
 * the sections f5 / f6 give the instance image value c*1000 + l.  Every other section belongs to no object, and a
 * NULL map gives zero objects.  (In a column without a terminator, which no compute call leaves, every one of the
 * max_sections slots counts, as is_render_sections paints them all.)  The image rows of a member are rows-1-vT .. rows-1-vB, clipped to the frame in
 * 64-bit arithmetic as is_render_sections clips; a member whose clipped rectangle is empty still counts as a stixel
 * (n_stixels, n_columns, the disparity fields, a contour point), contributes 0 pixels and leaves top / bottom alone.
 *
 * One is_instance_object per instance with at least one member, ascending by (frame, class, label):
 *   n_stixels          its members;  n_columns: the stixel columns that hold one;  col_min, col_max: the first and
 *                      last of them (image columns col_min*w .. col_max*w + w-1)
 *   top, bottom        smallest and largest clipped image row, inclusive; top = rows and bottom = -1 when no member
 *                      has a non-empty rectangle
 *   pixels             the sum over the members of clipped height * w (int32, wrapping).  For the well-formed columns
 *                      is_compute leaves this is exactly the area of draw_instance_masks' mask of the instance;
 *                      hand-built sections that overlap are counted once per SECTION, not once per pixel
 *   disparity_min/max  over the members whose disparity is not NaN, in the order of the order-preserving integer
 *                      mapping of fp32 (the fp32 order, with -0 below +0, so the bits do not depend on the order of
 *                      accumulation); +inf / -inf when every member is NaN
 *   disparity_q16_sum  the sum over the members of clipped height * llrint((double)d * 65536.0) for d in [0, 32768)
 *                      (which excludes NaN and the infinities; other d contribute 0), int64, wrapping.  The
 *                      pixel-weighted mean disparity is sum / (65536.0 * pixels / w)
 *   first_point        the index of its first contour point in d_points; its points are first_point ..
 *                      first_point + n_columns - 1
 * Every field is an integer sum, an integer extreme or an extreme over a total order: the bytes do not depend on the
 * order in which the device accumulates.
 *
 * One is_contour_point per (object, stixel column holding a member), ascending by (object, column): the member of
 * that column with the LARGEST disparity, i.e. the depth-closest one (z = focal * baseline / d) -- the same integer
 * order, NaN below everything, ties to the smaller section index.  (The reference's plot picks the closest by
 * Euclidean distance after a hard-coded Cityscapes filter; a host can recompute the 3-D position of every point from
 * (column, vB, vT, disparity), see instance_stixels_amd/world.py instance_objects.)  object: the index in d_objects;
 * section, vB, vT, disparity: of that member, bit for bit; column_pixels: the instance's pixels in that column. */
typedef struct is_instance_object {
    int32_t frame, semantic_class, label, n_stixels;
    int32_t n_columns, first_point, pixels, col_min;
    int32_t col_max, top, bottom, reserved; /* reserved = 0 */
    float disparity_min, disparity_max;
    int64_t disparity_q16_sum;
} is_instance_object;
typedef struct is_contour_point {
    int32_t object, column, section, vB;
    int32_t vT, column_pixels;
    float disparity;
    int32_t reserved; /* 0 */
} is_contour_point;
#ifdef __cplusplus
static_assert(sizeof(is_instance_object) == 64 && sizeof(is_contour_point) == 32, "16-byte chunks");
#else
_Static_assert(sizeof(is_instance_object) == 64 && sizeof(is_contour_point) == 32, "16-byte chunks");
#endif

/* Zero-initialise before setting fields.  All device arrays are on the current device.
 *   d_sections, d_section_instance, n_images, realcols, max_sections, rows, cols   as in is_render_args; the map
 *                       holds cluster labels or the ground-truth vote of f8; n_images in [1, 65535], max_sections in
 *                       [1, 32767] and n_images * realcols * max_sections < 2^31
 *   object_capacity, point_capacity   records d_objects / d_points hold (>= 0; the array may be NULL when it is 0)
 *   d_objects, d_points 16-byte aligned (the device writes 16-byte chunks): object r at index r for r <
 *                       object_capacity, point p at index p for p < point_capacity.  Nothing is written at or beyond
 *                       a capacity -- the caller sees the overflow in d_totals and repeats, as with is_stixel_world.
 *                       The two capacities are independent: a point below point_capacity is written even when its
 *                       object is not
 *   d_frame_objects, d_frame_points   [n_images] int32: the objects and points of every frame
 *   d_totals            [2] int32: the TRUE numbers of objects and points of the batch, also beyond the capacities */
typedef struct is_instance_objects_args {
    const is_section* d_sections;
    const int32_t* d_section_instance;
    int n_images, realcols, max_sections, rows, cols;
    int object_capacity, point_capacity;
    is_instance_object* d_objects;
    is_contour_point* d_points;
    int32_t* d_frame_objects;
    int32_t* d_frame_points;
    int32_t* d_totals;
} is_instance_objects_args;

/* The objects and contours of n_images frames on `stream`, asynchronously, without a host synchronisation: one memset
 * and four launches.  The scratch -- per frame 8000 keys x (40 bytes + one bit per stixel column), 33 MB for 64 frames
 * of 256 columns -- comes from the stream-ordered allocator and goes back to it on `stream`; a NULL map queues three
 * small memsets only. */
int is_instance_objects(const is_instance_objects_args* args, void* stream);

/* Thin wrappers over the HIP runtime so that the plain-C++ host class needs no HIP headers
 * (the reference's callers are all .cu files; ours may be plain C++). */
int is_device_malloc(void** ptr, size_t bytes);
int is_device_free(void* ptr);
int is_host_malloc(void** ptr, size_t bytes); /* pinned host memory */
int is_host_free(void* ptr);
int is_get_device(int* device);               /* the calling thread's current HIP device */
int is_set_device(int device);
int is_ctx_device(const is_ctx* ctx);         /* the device a context lives on */
int is_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream);
int is_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream);
/* `height` rows of `width` bytes from a pitched device array into a pitched (pinned) host array:
 * the host class fetches the first sections of every column this way instead of all max_sections */
int is_memcpy2d_d2h(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height,
                    void* stream);
int is_memset(void* dst, int value, size_t bytes, void* stream);
int is_stream_synchronize(void* stream);
/* A stream of the current device.  blocking != 0: an ordinary stream that still synchronises
 * implicitly with the legacy NULL stream, like every stream the reference's callers create
 * (cudaStreamCreate); 0: hipStreamNonBlocking. */
int is_stream_create(void** stream, int blocking);
int is_stream_destroy(void* stream);
int is_device_synchronize(void);

/* Test hook (A4, ComputeObjectLUT): copies the object data-cost prefix table of ONE stixel column
 * (0 <= column < n_images * realcols) as the last is_compute call on this context left it into
 * host memory, h_out[(rows + 1) * max_dis] = lutT[v][fn] -- the transpose of the reference's
 * d_object_lut[fn][v] (Stixels.cu:159-160, StixelsKernels.cu:959-978).  Synchronises the device.  After a unary call
 * that took the visited-rows walk (is_debug_unary_path: path 1) the buffer holds NO complete table: that call stores
 * only the table's block carries elsewhere and rebuilds the entries it reads; only the generic-encoding columns, and
 * every column of a repaired call, are complete. */
int is_debug_read_object_lut(is_ctx* ctx, int column, float* h_out);

/* Test hook: the block carries of the object table of ONE stixel column as the last walk call (is_debug_unary_path:
 * path 1) left them, h_out[ceil(rows / 32)][max_dis] = lutT[32 k][fn] (row 0 is zero).  A call on the tile path does
 * not write them.  Synchronises the device. */
int is_debug_read_lut_carries(is_ctx* ctx, int column, float* h_out);

/* Test hook: *on = 1 when the prepare step of the last is_compute / is_compute_sweep call of this context built the
 * carry rows with the kernel that keeps the cost table in LDS (walk calls with max_dis <= 128), 0 when it did not (tile
 * and pairwise calls, max_dis = 256), -1 before the first call; *pass_columns = the columns one pass of that kernel's
 * grid takes (a call with more columns runs its column loop more than once). */
int is_debug_lut_carry_lds(is_ctx* ctx, int* on, int* pass_columns);

/* Test hook: did the last unary is_compute call on this context run its repair launches?  A unary call whose every
 * tile is windowed builds the object data-cost table INSIDE its DP launch (the units of a column ahead of the
 * column's DP workgroups, which wait for a per-column count); a DP workgroup that cannot trust the hand-over -- its
 * column's units ran on another XCD than itself, or did not finish within the bound of its poll -- sets a word, and
 * the two launches queued behind (the ordinary table kernel and the ordinary DP launch, which otherwise leave at once)
 * do the call again.  *repaired = that word (0 in normal operation; IS_LUT_FUSED=2 forces 1 for tests, IS_LUT_FUSED=0
 * keeps the table in the prepare launch).  Synchronises the device. */
int is_debug_lut_fused_state(is_ctx* ctx, int* repaired);

/* The number of is_compute calls of this context whose repair launches have run since it was created (the reference
 * gets the order of its two launches from the stream, Stixels.cu:535-590; the fused launch has to earn it).  After the
 * first one the context plans its later calls with the table in the prepare launch again (unless IS_LUT_FUSED is set
 * to 1 or 2).  Synchronises the device. */
int is_lut_fused_repairs(is_ctx* ctx, int* calls_repaired);

/* Which unary DP the last unary is_compute call of this context ran: *path = 1 when it computed only the table rows
 * the back-trace visits (k_unary_path; IS_UNARY_PATH), 0 when it ran the tile path (every row),
 * -1 before the first unary call.  *repaired = the number of calls of this context whose path walk distrusted
 * itself and whose repair launches redid the call on the tile path.  Synchronises the device. */
int is_debug_unary_path(is_ctx* ctx, int* path, int* repaired);

/* Test hook: the bound-block summaries the pairwise DP of the last is_compute call left for one stixel
 * column (lemmas L7 / L8): h_out[n_blocks][24], returns n_blocks through *n_blocks. */
int is_debug_read_block_summaries(is_ctx* ctx, int column, float* h_out, int cap_floats, int* n_blocks);

/* Introspection used by bench.py / tests. */
const char* is_last_error(void);
const char* is_version(void);
/* Average duration (ms) of the DP kernel launches recorded by the last is_compute call on
 * this context, measured with HIP events on the launch stream; <0 if timing is disabled.  An
 * is_compute_sweep records none: after one, is_get_kernel_times_ms returns IS_EINVAL ("no call
 * recorded") until the next is_compute. */
int is_set_kernel_timing(is_ctx* ctx, int enabled);
int is_get_kernel_times_ms(is_ctx* ctx, float* prepare_ms, float* dp_ms, float* backtrace_ms);
size_t is_scratch_bytes(const is_ctx* ctx);
/* Evaluation counters of the exact branch-and-bound, for measurements
 * OUTSIDE a timed region: while enabled, the DP kernels of FAST columns add the number of 64-pair
 * wave-steps they evaluated below the diagonal blocks to a device array (enabling resets it).
 *   out[0] unary full steps, out[1] unary ground/sky-only steps,
 *   out[2] pairwise phase-1 full steps, out[3] pairwise phase-1 ground/sky-only candidates,
 *   out[4] pairwise phase-1 steps in which some lane read OUTSIDE its fn window (window misses),
 *   out[5] the same for the unary ring kernel; out[6] / out[7]: the fused LUT units of the unary launch (polls of
 *   waiting DP workgroups / shader clocks the units lived);
 *   out[8 + 3 t + j], t < 64: the phase-1 launch of 64-row tile t alone, j = 0 full, 1 window
 *   misses, 2 ground/sky-only.  n <= IS_EVAL_COUNTERS.  Both calls synchronise the device. */
#define IS_EVAL_COUNTERS 200
int is_set_eval_counters(is_ctx* ctx, int enabled);
int is_get_eval_counters(is_ctx* ctx, unsigned long long* out, int n);

#ifdef __cplusplus
}
#endif

#endif /* INSTANCE_STIXELS_CORE_H_ */
