/*
 * Stixels.hpp -- host class of the MI355X-native stixel library.
 *
 * Public surface = the reference's `class Stixels`
 * (/root/reference/InstanceStixels/include/InstanceStixels/Stixels.hpp:40-96): same method
 * names, argument meaning and error behaviour, so run_cityscapes / StixelsWrapper / the ROS node
 * compile against it unchanged.  Differences, all behind the same API:
 *   - plain C++ header (no CUDA/HIP types): callers need not be device translation units;
 *   - the device side is the C ABI of include/instance_stixels_core.h (HIP, gfx950);
 *   - Compute() does not modify the segmentation buffer it is given;
 *   - ComputeBatch() / InitializeBatch() are additions for batched, multi-GPU use.
 */
#ifndef INSTANCESTIXELS_AMD_STIXELS_HPP_
#define INSTANCESTIXELS_AMD_STIXELS_HPP_

#include <stdint.h>

#include <cmath>
#include <map>
#include <utility>
#include <vector>

#include "configuration.h"
#include "types.h"
#include "util.h"

constexpr float PIFLOAT = 3.1416f;

/* Every DeviceArray / PinnedArray of a Stixels object (its private base: the members keep their plain names).
 * Stixels::Finish() releases them with release_all(), which stands at the end of the declarations; the static_assert
 * behind the struct counts the members, so an array added here and not released there does not compile. */
struct StixelsBuffers {
    DeviceArray<pixel_t> d_disparity;
    DeviceArray<pixel_t> d_disparity_big;
    DeviceArray<int32_t> d_segmentation;
    DeviceArray<float> d_instance_centerofmass;
    DeviceArray<int32_t> d_instance_indices;
    DeviceArray<uint8_t> d_instance_core_candidates;
    /* (every instance array: one slice per frame of the batch) */
    DeviceArray<int32_t> d_instance_labels;  /* the reference's d_instance_labels, Stixels.cu:66-68 */
    DeviceArray<int32_t> d_instance_packed;  /* [1 + 3*classes*realcols*max_sections], see is_instance_buffers */
    /* pinned host mirrors: Compute() ends with ONE stream synchronisation */
    PinnedArray<Section> h_stixels;
    /* One device block: header rows (the per-class candidate counts, d_instances_per_class) in
     * front of the sections (d_stixels), both aliases into it set by InitializeBatch.  Compute()
     * fetches the header and the first m_head_sections sections of every column with ONE pitched
     * copy into h_stixels_head; a column without a terminator among them (rare) makes it fetch the
     * complete array. */
    DeviceArray<Section> d_stixels_block;
    PinnedArray<Section> h_stixels_head;
    PinnedArray<int32_t> h_instance_head;    /* [max_batch][8 per-class counts] */
    /* ComputeBatchGather: the packed payload of this rank and, on the destination, the landing buffers
     * (allocated on first use, grown on demand, released by Finish) */
    DeviceArray<int32_t> d_pack_counts;
    DeviceArray<int32_t> d_pack_offsets;
    DeviceArray<Section> d_pack_sections;
    DeviceArray<int32_t> d_all_counts;
    DeviceArray<Section> d_all_packed;
    /* ComputeBatch: the same packed payload copied to the host in two pinned pieces (offsets, used sections) */
    PinnedArray<int32_t> h_pack_offsets;
    PinnedArray<Section> h_pack_sections;
    PinnedArray<int32_t> h_all_counts; /* ComputeBatchGather on dst: the per-column counts of all ranks */
    PinnedArray<int32_t> h_instance_packed;
    /* RenderBatch: the per-section label map and the per-frame results (allocated on first use) */
    DeviceArray<int32_t> d_section_instance; /* [max_batch][realcols][max_sections] */
    /* AssignInstancesGTBatch: the ground-truth map of the same shape; the packed (frame, column, section, label)
     * quads behind their count, device and pinned host */
    DeviceArray<int32_t> d_section_instance_gt;
    DeviceArray<int32_t> d_section_instance_gt_packed; /* [4 + 4 * sections of the batch], is_pack_section_labels */
    PinnedArray<int32_t> h_section_instance_gt;
    DeviceArray<char> d_render_results;      /* [max_batch] double | [max_batch] int64 | [max_batch] int32 */
    PinnedArray<char> h_render_results;
    /* InstanceOverlapBatch: [max_batch][capacity] records, then n_records | overflow per frame, the packed records
     * (device and pinned host, allocated on first use, grown with the capacity) */
    DeviceArray<is_overlap_record> d_overlap_records;
    DeviceArray<is_overlap_record> d_overlap_packed;
    DeviceArray<int32_t> d_overlap_header;   /* [max_batch] n_records | [max_batch] overflow */
    PinnedArray<int32_t> h_overlap_header;
    PinnedArray<is_overlap_record> h_overlap_packed;
    /* WorldBatch: the per-column counts and offsets, the frame totals and the records (device and pinned host,
     * allocated on first use, grown on demand) */
    DeviceArray<int32_t> d_world_counts;   /* [max_batch * realcols] */
    DeviceArray<int32_t> d_world_offsets;  /* [max_batch * realcols + 1] */
    DeviceArray<int32_t> d_world_totals;   /* [max_batch] */
    DeviceArray<is_world_stixel> d_world;
    PinnedArray<int32_t> h_world_totals;
    PinnedArray<is_world_stixel> h_world;
    /* InstanceObjectsBatch: one device block and its pinned mirror, laid out
     * [2] totals | [max_batch] frame objects | [max_batch] frame points | objects | points (16-byte aligned parts),
     * so that one copy brings everything */
    DeviceArray<char> d_objects_block;
    PinnedArray<char> h_objects_block;
    /* SweepBatch: the Sections of [sets][frames] and one block of their instance arrays, frame after frame (per-class
     * counts | centres | indices | labels | packed triples | core flags, see Stixels::SweepInstanceBuffers); allocated
     * on first use, grown on demand */
    DeviceArray<Section> d_sweep_stixels;
    DeviceArray<char> d_sweep_instances;
    /* ClusterInstanceDisparityBatch: the core's scratch, the two images of a call whose inputs are host arrays, and
     * [max_batch] key counts | the stixel medians of the batch (device and pinned host; allocated on first use) */
    DeviceArray<char> d_idisp_scratch;
    DeviceArray<char> d_idisp_inputs;
    DeviceArray<char> d_idisp_out;
    PinnedArray<char> h_idisp_out;
    /* GroundTruthOffsetsBatch: the core's scratch (allocated on first use) */
    DeviceArray<char> d_gt_targets_scratch;
    /* ComputeBatchRoad: [max_batch] RoadParameters | [max_batch] status bytes, the copy of the caller's device arrays */
    PinnedArray<char> h_road;
    /* SegmentationHeadBatch: [channels][K] weights | [channels] bias of SetSegmentationHead (uploaded on first use) */
    DeviceArray<float> d_head_weights;
    void release_all() { /* in the order of the declarations */
        d_disparity.release(); d_disparity_big.release(); d_segmentation.release(); d_instance_centerofmass.release();
        d_instance_indices.release(); d_instance_core_candidates.release(); d_instance_labels.release();
        d_instance_packed.release(); h_stixels.release(); d_stixels_block.release(); h_stixels_head.release();
        h_instance_head.release(); d_pack_counts.release(); d_pack_offsets.release(); d_pack_sections.release();
        d_all_counts.release(); d_all_packed.release(); h_pack_offsets.release(); h_pack_sections.release();
        h_all_counts.release(); h_instance_packed.release(); d_section_instance.release();
        d_section_instance_gt.release(); d_section_instance_gt_packed.release(); h_section_instance_gt.release();
        d_render_results.release(); h_render_results.release(); d_overlap_records.release();
        d_overlap_packed.release(); d_overlap_header.release(); h_overlap_header.release(); h_overlap_packed.release();
        d_world_counts.release(); d_world_offsets.release(); d_world_totals.release(); d_world.release();
        h_world_totals.release(); h_world.release(); d_objects_block.release(); h_objects_block.release();
        d_sweep_stixels.release(); d_sweep_instances.release(); d_idisp_scratch.release(); d_idisp_inputs.release();
        d_idisp_out.release(); h_idisp_out.release(); d_gt_targets_scratch.release(); h_road.release();
        d_head_weights.release();
    }
};
static_assert(sizeof(StixelsBuffers) == 49 * sizeof(DeviceArray<char>), "release_all() must release every array");

class Stixels : private StixelsBuffers {
public:
    Stixels();
    ~Stixels();

    void Initialize();
    void Finish();

    float Compute(bool pairwise, StixelsData& stixels, int32_t* d_segmentation_local = nullptr);
    float ClusterInstances();
    std::map<std::pair<int, int>, int> GetInstanceStixels();
    int GetRealCols();
    int GetMaxSections();
    void SetConfig(const StixelConfig& config);
    void SetSegmentation(const std::vector<int32_t>& segmentation);
    void SetSegmentationParameters(const int classes, const int instance_channels);
    void SetClusteringParameters(const float eps, const int min_pts, const int size_filter);
    void SetWeightParameters(const float prior_weight, const float disparity_weight,
                             const float segmentation_weight, const float instance_weight);
    void SetDisparityImage(const std::vector<pixel_t>& disp_im);
    pixel_t* GetInputDisparityImageOnDevice();
    void SetProbabilities(float pout, float pout_sky, float pground_given_nexist,
                          float pobject_given_nexist, float psky_given_nexist, float pnexist_dis,
                          float pground, float pobject, float psky, float pord, float pgrav,
                          float pblg);
    void SetRoadParameters(int vhor, float camera_tilt, float camera_height, float alpha_ground);
    void SetCameraParameters(float focal, float baseline, float sigma_camera_tilt,
                             float sigma_camera_height, float camera_center_x = -1,
                             float camera_center_y = -1);
    void SetDisparityParameters(const int rows, const int cols, const int max_dis,
                                const float invalid_disparity, const float sigma_disparity_object,
                                const float sigma_disparity_ground, float sigma_sky);
    void SetModelParameters(const int column_step, const bool median_join, float epsilon,
                            float range_objects_z, int width_margin);
    std::vector<float> Get3DVertices(const StixelsData& stixels_data);
    static void SaveStixels(Section* stixels, std::map<std::pair<int, int>, int> instance_stixels,
                            const float alpha_ground, const int vhor, const int real_cols,
                            const int max_segments, const char* fname);
    bool IsInitialized() { return m_is_initialized; }

    /* ---- additions (not in the reference) ---- */
    /* Road parameters of one frame of a batch, image-convention vhor as in SetRoadParameters. */
    struct RoadParameters {
        int vhor;
        float camera_tilt, camera_height, alpha_ground;
    };
    /* Device the next Initialize() creates its buffers on; default (-1): the calling thread's
     * current HIP device at Initialize() time (one process per GPU: select the device before, as
     * with the reference's CUDA code).  Every later call runs on that device whatever the
     * caller's current device is. */
    void SetDevice(int device) { m_device = device; }
    /* the device requested with SetDevice() (-1 = current device at Initialize() time) */
    int GetDevice() const { return m_device; }
    /* the device the buffers of the last Initialize() live on (-1 before) */
    int GetActiveDevice() const { return m_ctx_device; }
    /* Host half of Initialize() (tables + parameter block); needs no device. */
    void PrecomputeHost();
    /* Like Initialize(), with device scratch for up to max_batch frames per ComputeBatch(). */
    void InitializeBatch(int max_batch);
    /* Batched Compute on device-resident inputs:
     *   d_disparity_big [n][rows][cols] float, d_segmentation [n][realcols][channels][P2S] int32.
     * Fills `out[i]` like Compute() fills its StixelsData.  `stream` is a hipStream_t.
     * `instance_stixels` (optional): filled with what GetInstanceStixels() returns after a
     * Compute() of frame i -- the instance candidates of every frame are compacted and clustered
     * on the device in two launches for the whole batch (the reference does both inside
     * Compute(), StixelsKernels.cu:926-942, Stixels.cu:613). */
    typedef std::map<std::pair<int, int>, int> InstanceMapping;
    void ComputeBatch(bool pairwise, int n_images, const pixel_t* d_disparity_big,
                      const int32_t* d_segmentation, const RoadParameters* road,
                      std::vector<StixelsData>& out, void* stream = nullptr,
                      std::vector<InstanceMapping>* instance_stixels = nullptr);
    /* ComputeBatch with the road parameters left on the device (an addition): d_road [n_images] RoadParameters and
     * d_status [n_images] uint8, device, e.g. as RoadEstimation::ComputeBatchDevice queued them on the same stream.
     * The ground model of every frame is built on the device (is_compute_road) -- nothing is computed per row on the
     * host, and the chain disparity -> lines -> road -> ground model -> DP has no synchronisation before the one
     * that delivers the Sections.  d_road and d_status come back in one small pinned copy behind the DP: the header
     * of every StixelsData and every consumer of the batch (RenderBatch, WorldBatch, ...) take alpha_ground and vhor
     * from it; road_out / status_out (optional) receive them.  A frame whose status is not IS_ROAD_OK was computed
     * with the fallback record ComputeBatchDevice put in its place.
     * The ground model is PrecomputeGroundShared's, bit for bit: is_erff in place of erff, everything else as
     * PrecomputeGround (DESIGN.md 10j states the distance to ComputeBatch). */
    void ComputeBatchRoad(bool pairwise, int n_images, const pixel_t* d_disparity_big, const int32_t* d_segmentation,
                          const RoadParameters* d_road, const uint8_t* d_status, std::vector<StixelsData>& out,
                          void* stream = nullptr, std::vector<InstanceMapping>* instance_stixels = nullptr,
                          std::vector<RoadParameters>* road_out = nullptr,
                          std::vector<uint8_t>* status_out = nullptr);
    /* The host twin of the device ground model (k_ground_model), without a device: PrecomputeGround with is_erff of
     * is_numerics.h in place of erff and the FastLog index clamped to the table, row for row is_ground_row of
     * is_ground_model.h.  function / normalization / inv_sigma2: [rows]; range_index (may be null): [rows], the
     * FastLog index of the a_range term. */
    static void PrecomputeGroundShared(const is_ground_params& g, const float* log_lut, int lut_entries, int rows,
                                       int vhor_lib, float camera_tilt, float camera_height, float alpha_ground,
                                       float* function, float* normalization, float* inv_sigma2,
                                       int* range_index = nullptr);
    /* the constants of the ground model as this object holds them, and its FastLog table (after PrecomputeHost()) */
    is_ground_params GroundParams() const;
    const std::vector<float>& GetLogLUT() const { return m_log_lut; }
    /* Multi-GPU (an addition: the reference runs on one GPU): this rank's shard of a batch through
     * ComputeBatch's device path, then the compacted final gather of EVERY rank's Sections on rank `dst` of
     * `comm` over RCCL (an ncclComm_t passed as void*; plain-C++ callers create it with is_comm_unique_id /
     * is_comm_init_rank of instance_stixels_core.h).  One process per GPU, every rank calls it.
     *   images_per_rank  [ranks]: the shard sizes, known to every rank; n_images = its own entry
     *   road_all         on dst: the road parameters of ALL frames in rank order (dst hands out the work,
     *                    so it has them) for the StixelsData headers; ignored elsewhere
     * On dst `out` holds the frames of all ranks in rank order, elsewhere it is left empty.  Sections
     * only: the instance mappings stay with the rank that computed them (ComputeBatch). */
    void ComputeBatchGather(bool pairwise, int n_images, const pixel_t* d_disparity_big,
                            const int32_t* d_segmentation, const RoadParameters* road, void* comm, int dst,
                            const int* images_per_rank, const RoadParameters* road_all,
                            std::vector<StixelsData>& out, void* stream = nullptr);
    /* f5 (an addition): the Sections of frames 0 .. n_images-1 of the LAST Compute() or ComputeBatch() -- both
     * leave them in d_stixels, their cluster labels in d_instance_labels -- rendered to dense per-pixel result
     * maps and scored against ground truth on the device, as is_render_sections of instance_stixels_core.h
     * defines every field (all device pointers on the object's device; NULL = skipped). */
    struct RenderTargets {
        uint8_t* label = nullptr;           /* [n][rows][cols] labelIds (class_to_label of the section class) */
        float* disparity = nullptr;         /* [n][rows][cols] section disparity */
        int32_t* instance = nullptr;        /* [n][rows][cols] class*1000 + cluster label; needs instances */
        const uint8_t* gt_label = nullptr;  /* [n][rows][cols], with confusion */
        int n_labels = 34;
        unsigned long long* confusion = nullptr; /* [n_labels][n_labels], added to */
        const float* gt_disparity = nullptr;     /* [n][rows][cols]: the deviation of RenderResult */
        const uint8_t* class_to_label = nullptr; /* host [n_classes]; NULL: Cityscapes trainId -> labelId */
        int n_classes = 0;
    };
    struct RenderResult {
        double disp_abs_sum;   /* sum of |stixel - gt| over pixels where both are non-zero (0 without gt) */
        int64_t disp_count;
        int32_t stixel_count;  /* sections in front of the terminators */
    };
    /* Queues the render on `stream` (null: the object's own), then ONE small copy and a synchronisation for the
     * per-frame results.  Throws std::invalid_argument before any compute, when n_images exceeds the last call's
     * batch, or when an instance image is asked of a call that ran without instances. */
    std::vector<RenderResult> RenderBatch(int n_images, const RenderTargets& targets, void* stream = nullptr);
    /* f6 (an addition): per frame 0 .. n_images-1 of the LAST Compute() or ComputeBatch(), the sparse joint
     * histogram of its instance image (RenderTargets::instance, never rendered) and d_gt_instance [n][rows][cols]
     * int32 Cityscapes instanceIds, as is_instance_overlap defines it: {pred, gt, count} ascending by (pred, gt),
     * every table complete (a frame that overflows the initial capacity is repeated alone with a larger one, up to
     * rows*cols).  One packed copy of the used records.  Throws std::invalid_argument before any compute under
     * RenderBatch's rules, and when the last call ran without instances. */
    std::vector<std::vector<is_overlap_record>> InstanceOverlapBatch(int n_images, const int32_t* d_gt_instance,
                                                                     void* stream = nullptr);
    /* Records per frame of InstanceOverlapBatch's first pass (default 4096; [1, IS_OVERLAP_MAX_CAPACITY]). */
    void SetInstanceOverlapCapacity(int records);
    /* f7 (an addition): the 3-D stixel world of frames 0 .. n_images-1 of the LAST Compute() or ComputeBatch() --
     * per stixel one is_world_stixel (instance_stixels_core.h): its Section fields, its column and index, the
     * cluster label GetInstanceStixels() gives it (-1: none; every id is -1 after a call without instances) and the
     * twelve floats Get3DVertices() gives it, for the road parameters of that call.  Frame f's records are
     * stixels[frame_offsets[f] .. frame_offsets[f + 1]), in (column, section) order.  Built on the device and
     * brought to the host compacted: the frame totals, then exactly the used records, through pinned memory.
     * Throws std::invalid_argument before any compute under RenderBatch's rules, and "Camera parameters are not
     * set." under Get3DVertices' condition.  (A column WITHOUT a terminator, which no compute call leaves, gives
     * max_sections - 1 records, as is_pack_sections packs it, where Get3DVertices walks all max_sections slots.) */
    struct World {
        std::vector<int32_t> frame_offsets; /* [n_images + 1] */
        std::vector<is_world_stixel> stixels;
    };
    /* By value: every call allocates the result anew.  At batch 64 of 1024x2048 that is ~89 MB of fresh pages per
     * call, and this form then measured SLOWER than the host composition it replaces: a
     * caller that runs batch after batch uses one of the two forms below. */
    World WorldBatch(int n_images, void* stream = nullptr);
    /* The same into a caller's World, whose vectors keep their capacity from call to call: one copy out of the
     * pinned buffer into warm pages per batch. */
    void WorldBatch(int n_images, World& world, void* stream = nullptr);
    /* The same without that copy: the records where the device-to-host copy left them, in the object's pinned
     * buffer, readable until the next WorldBatch*() or Finish() of this object (what ish_world_batch and the
     * Python binding read, straight into the caller's array).  frame_offsets: [n_images + 1]. */
    const is_world_stixel* WorldBatchView(int n_images, std::vector<int32_t>& frame_offsets, void* stream = nullptr);
    /* n records from a view into the caller's array: the copy of WorldBatch(n, world), split over up to 8 host
     * threads from 8 MB on (one thread copies a 64-frame batch in ~3.4 ms, longer than the device takes to build
     * and deliver it). */
    static void CopyWorldRecords(is_world_stixel* dst, const is_world_stixel* src, size_t n);
    /* Records per frame the device buffer of WorldBatch's first pass holds.  Without it (and again after
     * SetWorldCapacity(0)) the buffer has the exact size where the last call was a ComputeBatch (which has counted
     * its sections; then the totals and the records travel behind ONE synchronisation) and 4096 records per frame
     * after a Compute().  A batch that needs more is repeated with its true total: the result is always complete. */
    void SetWorldCapacity(int records_per_frame);
    /* f8 (an addition): the instance id of every stixel of frames 0 .. n_images-1 of the LAST Compute() or
     * ComputeBatch() by majority vote over d_gt_instance [n][rows][cols] int32 (Cityscapes instanceIds), as
     * is_assign_instances_gt defines it -- the reference tooling's assign_instances_gt (--use-instancegt), the
     * upper bound of its instance evaluation.  The vote needs no instance candidates: it works after a compute call
     * without instance outputs too.  It fills a second per-section map of the object, and from then on RenderBatch,
     * InstanceOverlapBatch and WorldBatch* take their instance ids from that map (frames the vote did not cover have
     * none) until the next compute call or UseClusterInstances().  `mapping`, when given, receives per frame
     * (column, section) -> label of every labelled section, in one packed copy behind one synchronisation.  Throws
     * std::invalid_argument under RenderBatch's rules (before any compute, n_images beyond the last batch). */
    void AssignInstancesGTBatch(int n_images, const int32_t* d_gt_instance, void* stream = nullptr,
                                std::vector<InstanceMapping>* mapping = nullptr);
    /* f11 (an addition): the two offset channels of a DP input from the ground truth, the producer of the reference's
     * "gt offsets" row (--usegtoffsets of tools/run_cityscapes.py: inference.py:388-396 with the 1/8-resolution
     * targets of its training, datasets/cityscapes.py:146-167), as is_gt_instance_targets defines it.  Channels 19 and
     * 20 of d_segmentation [n_images][cols / 8][21][rows_power2_segmentation] int32 are rewritten from d_gt_instance
     * [n_images][rows][cols] int32 with the object's rows and cols, padding rows included; the class channels are not
     * touched.  It is a producer like the CNN wrapper: valid before any compute call, asynchronous on `stream`, and
     * it leaves the record of the last batch alone.  Throws std::invalid_argument for n_images outside [1, max_batch],
     * a null pointer, or rows / cols that are no multiples of 8. */
    void GroundTruthOffsetsBatch(int n_images, const int32_t* d_gt_instance, int32_t* d_segmentation,
                                 void* stream = nullptr);
    /* f13 (an addition): the CNN's segmentation head, the last layers of the reference's models and its export
     * wrapper (DRNDownsampled.py:97-102 and :128-137, wrappers.py:35-61), as is_segmentation_head defines it.
     * SetSegmentationHead takes `seg.weight` [channels][K] and `seg.bias` [channels] of the 1x1 convolution, channels
     * = the classes + instance channels of SetSegmentationParameters; throws std::invalid_argument unless bias.size()
     * is that number, weight.size() == bias.size() * K and K >= 8 is a multiple of 8.  Needs no device: the object
     * keeps the values and uploads them on the first SegmentationHeadBatch after Initialize. */
    void SetSegmentationHead(const std::vector<float>& weight, const std::vector<float>& bias, int K);
    /* The clamp of one regression channel (DRNDSOffsetDisparity's disparity channel: [0, 128]); channel -1: none
     * (the default).  Throws std::invalid_argument unless lo <= hi. */
    void SetSegmentationHeadClamp(int channel, float lo, float hi);
    /* d_features [n_images][K][rows / 8][realcols] of dtype IS_HEAD_F32 / _F16 / _BF16 (backbone output, contiguous
     * NCHW) -> d_segmentation [n_images][realcols][channels][rows_power2_segmentation] int32, what ComputeBatch,
     * ComputeBatchRoad and SweepBatch take, and optionally d_cnn_out [n_images][channels][rows / 8][realcols] fp32.
     * rows / 8, realcols, the channel split and rows_power2_segmentation are the initialised object's, so a caller
     * cannot mismatch them.  A producer like GroundTruthOffsetsBatch: valid before any compute call, one asynchronous
     * launch on `stream`, the record of the last batch untouched.  Throws std::invalid_argument before
     * SetSegmentationHead, for n_images outside [1, max_batch] and for what is_segmentation_head refuses. */
    void SegmentationHeadBatch(int n_images, const void* d_features, int dtype, int32_t* d_segmentation,
                               float* d_cnn_out = nullptr, void* stream = nullptr);
    /* f15 (an addition): the CNN's own label image of a batch at full resolution and its confusion table, the row the
     * reference's evaluation prints beside the stixels' (tools/run_cityscapes.py:353-365, 551), as is_cnn_label_maps
     * defines it.  d_cnn_out [n_images][channels][rows / 8][realcols] fp32 is SegmentationHeadBatch's float output;
     * mode is IS_CNN_UP_NEAREST or IS_CNN_UP_DECONV.  rows, cols, rows / 8, realcols and the channel split are the
     * initialised object's, so a caller cannot mismatch them.  A producer like SegmentationHeadBatch: valid before any
     * compute call, one asynchronous launch on `stream`, the record of the last batch untouched.  Throws
     * std::invalid_argument for n_images outside [1, max_batch] and for what is_cnn_label_maps refuses. */
    struct CnnLabelTargets {
        uint8_t* class8 = nullptr;          /* [n][rows / 8][realcols]: the class of every cell */
        uint8_t* label = nullptr;           /* [n][rows][cols] labelIds (Cityscapes trainId -> labelId) */
        const uint8_t* gt_label = nullptr;  /* [n][rows][cols], with confusion */
        int n_labels = 34;
        unsigned long long* confusion = nullptr; /* [n_labels][n_labels], added to */
    };
    void CnnLabelBatch(int n_images, const float* d_cnn_out, int mode, const CnnLabelTargets& targets,
                       void* stream = nullptr);
    /* Back to the cluster labels of the last compute call. */
    void UseClusterInstances() { m_last.gt_instances = false; }
    /* The vote's parameters (defaults: the reference's): the minimum fraction of the 10 % rule, the labelIds of
     * classes 11..18 (null: Cityscapes 24, 25, 26, 27, 28, 31, 32, 33), and whether the ground truth is in trainId
     * form (class*1000 + k, *_instanceTrainIds.png).  Throws std::invalid_argument on a NaN fraction or an id outside
     * [0, 2147482]. */
    void SetGTAssignmentParameters(double min_fraction, const int* label_ids8, bool gt_is_train_ids);
    /* f9 (an addition): the per-INSTANCE form of frames 0 .. n_images-1 of the LAST Compute() or ComputeBatch(), as
     * is_instance_objects (instance_stixels_core.h) defines every field: one is_instance_object per (frame, class,
     * label) that has a stixel, ascending, and per object one is_contour_point per stixel column it touches -- the
     * depth-closest stixel of the instance in that column -- at points[first_point .. first_point + n_columns).  The
     * instance ids are those the three consumers above read: the cluster labels, or the ground-truth vote after
     * AssignInstancesGTBatch; after a call without instances the batch has no objects.  A few kilobytes per frame
     * where WorldBatch moves megabytes.  Built on the device; the totals, the per-frame counts and the records reach
     * pinned memory behind ONE synchronisation (a batch beyond the capacities is repeated once with its true totals,
     * and the object keeps the larger buffers).  Throws std::invalid_argument under RenderBatch's rules. */
    struct InstanceObjects {
        std::vector<int32_t> frame_objects, frame_points; /* [n_images] each */
        std::vector<is_instance_object> objects;
        std::vector<is_contour_point> points;
    };
    /* The records where the copy left them, in the object's pinned buffer: readable until the next
     * InstanceObjectsBatch*() or Finish() of this object. */
    struct InstanceObjectsView {
        const int32_t* frame_objects; /* [n_images] */
        const int32_t* frame_points;  /* [n_images] */
        const is_instance_object* objects;
        const is_contour_point* points;
        int32_t n_objects, n_points;
    };
    InstanceObjectsView InstanceObjectsBatchView(int n_images, void* stream = nullptr);
    /* The same copied into a caller's InstanceObjects, whose vectors keep their capacity from call to call. */
    void InstanceObjectsBatch(int n_images, InstanceObjects& out, void* stream = nullptr);
    /* Objects per frame the first pass has room for (default 64; [1, 8000]); the points get 8 per object. */
    void SetInstanceObjectCapacity(int objects_per_frame);
    /* Parameter sweeps (an addition): what the reference's hyper-parameter search (tools/run_cityscapes.py:566-680)
     * changes between two runs over the same frames -- the four weights in SetWeightParameters' user-facing form (the
     * class applies its instance / segmentation rule) and the three clustering parameters. */
    struct SweepSet {
        float prior_weight, disparity_weight, segmentation_weight, instance_weight;
        float eps;
        int min_pts, size_filter;
    };
    /* the set as the core takes it: SetWeightParameters' rule for the instance weight */
    static is_sweep_set CoreSweepSet(const SweepSet& set);
    /* ComputeBatch for every set of `sets` on the same inputs in one call (is_compute_sweep): the column join and the
     * ground models run once, the weight-independent half of the DP once, the rest per set.  The results stay on the
     * device, in arrays the object allocates on first use and grows by the Sections and the instance arrays of
     * sets x n_images frames (never by DP scratch); nothing is copied to the host.  Afterwards set 0 is "the last batch"
     * of the consumers (RenderBatch, InstanceOverlapBatch, WorldBatch*, AssignInstancesGTBatch, InstanceObjectsBatch*);
     * SelectSweepSet chooses another.  The object's own parameters are unchanged.  Throws std::invalid_argument, before
     * anything is queued, when n_images is outside [1, max_batch] or `sets` is empty. */
    void SweepBatch(bool pairwise, int n_images, const pixel_t* d_disparity_big, const int32_t* d_segmentation,
                    const RoadParameters* road, const std::vector<SweepSet>& sets, void* stream = nullptr,
                    bool with_instances = true);
    /* Makes set k of the last SweepBatch what the consumers read (no copy).  Throws std::invalid_argument when k is
     * outside the sets of that call, or when the last compute call was not a sweep (Compute, ComputeBatch,
     * ComputeBatchGather and Finish end it). */
    void SelectSweepSet(int k);
    /* One set of the last SweepBatch to the host, as ComputeBatch delivers a batch (packed on the device, through
     * pinned memory); `instance_stixels` needs a sweep with instances.  Throws like SelectSweepSet. */
    void SweepSections(int k, std::vector<StixelsData>& out, std::vector<InstanceMapping>* instance_stixels = nullptr);
    /* The clustering of the last compute call -- or of the selected set of a sweep -- again with other parameters,
     * without its DP (is_recluster): the labels (and `instance_stixels`, when given) are afterwards those of a compute
     * call made with these three parameters, the Sections untouched.  Ends an active ground-truth map, as
     * UseClusterInstances does.  Throws std::invalid_argument before any compute call and after one without
     * instances. */
    void ReclusterBatch(float eps, int min_pts, int size_filter, std::vector<InstanceMapping>* instance_stixels = nullptr,
                        void* stream = nullptr);
    /* f10 (an addition): the instance ids of frames 0 .. n_images-1 of the last compute call -- or of the selected set
     * of a sweep -- by the size-filtered DBSCAN over (instance_mean_x, instance_mean_y, instance disparity), the
     * reference tooling's --use-disparity from_gt, as is_cluster_instance_disparity defines every step: the median
     * disparity of every ground-truth instance, its median over every instance-class stixel, and the clustering in
     * which the stixels whose median is 0 take no part.  gt_instance [n][rows][cols] int32 (Cityscapes instanceIds)
     * and disparity_u8 [n][rows][cols] uint8 are device arrays, or host arrays with inputs_on_host (copied into the
     * object's own buffers).  The labels of the frames are rewritten as ReclusterBatch rewrites them, so
     * GetInstanceStixels, RenderBatch, InstanceOverlapBatch, WorldBatch* and InstanceObjectsBatch* see them; an active
     * ground-truth map ends.  `instance_stixels`, when given, receives the mappings; `stixel_median`, when given, is a
     * host array [n_images][realcols][max_sections] that receives every stixel's median.  The call synchronises once
     * (it reads the frames' key counts).  Throws std::invalid_argument under RenderBatch's rules and after a compute
     * call without instances, and std::runtime_error, with every label unchanged, when a frame holds more
     * ground-truth instances than SetInstanceDisparityCapacity allows. */
    void ClusterInstanceDisparityBatch(int n_images, const int32_t* gt_instance, const uint8_t* disparity_u8, float eps,
                                       int min_pts, int size_filter,
                                       std::vector<InstanceMapping>* instance_stixels = nullptr,
                                       float* stixel_median = nullptr, void* stream = nullptr,
                                       bool inputs_on_host = false);
    /* Ground-truth instances (keys) per frame ClusterInstanceDisparityBatch has histogram slots for, 1 KiB each
     * (default 256); throws std::invalid_argument outside [1, IS_INSTANCE_DISPARITY_KEYS]. */
    void SetInstanceDisparityCapacity(int keys_per_frame);
    /* frames of the last compute call the consumers can read (0: none) */
    int LastFrames() const { return m_last.frames; }
    /* sets of the last SweepBatch while it is what the consumers read (0: the last compute call was not a sweep) */
    int SweepSets() const { return m_sweep.sets; }
    /* Introspection for tests / bench. */
    const StixelParameters& GetParameters() const { return m_params; }
    const std::vector<float>& GetObjectCostLUT() const { return m_obj_cost_lut; }
    const std::vector<float>& GetObjectDisparityRange() const { return m_object_disparity_range; }
    void GetGroundModel(std::vector<float>& ground_function,
                        std::vector<float>& normalization_ground,
                        std::vector<float>& inv_sigma2_ground, int& vhor_lib);
    is_ctx* GetCoreContext() { return m_ctx; }

private:
    struct GroundModel {
        std::vector<float> function, normalization, inv_sigma2;
    };
    void PrecomputeSky();
    void PrecomputeObject();
    void PrecomputeGround(int vhor_lib, float camera_tilt, float camera_height, float alpha_ground,
                          GroundModel& out) const;
    float GetDataCostObject(const int fn, const int dis) const;
    float ComputeObjectDisparityRange(const float previous_mean) const;
    float FastLog(float v) const;
    void FillHeader(StixelsData& d, float alpha_ground, int vhor_lib) const;
    /* the ground models of frames 0 .. n_images-1 end to end ([n][rows] each) and their library-convention vhor */
    void BatchGround(int n_images, const RoadParameters* road, GroundModel& batch, std::vector<int>& vhor) const;
    /* packed Sections (counts[frame * realcols + column] per column, in order) into the fixed-stride sections of
     * the frames in `out`, each column closed by a terminator */
    void ScatterSections(const int32_t* counts, const Section* packed, size_t total,
                         std::vector<StixelsData>& out) const;
    void ReservePackBuffers();
    /* The second half of ComputeBatch and ComputeBatchRoad: the Sections of the batch in d_stixels (and the instance
     * mappings) to the host.  `road` [n_images] is read behind the first synchronisation (ComputeBatchRoad passes
     * the pinned copy queued in front); remember: that is also where the batch is recorded for the consumers. */
    void DeliverBatch(int n_images, const RoadParameters* road, bool remember, std::vector<StixelsData>& out,
                      void* stream, std::vector<InstanceMapping>* instance_stixels);
    is_instance_buffers InstanceBuffers(int image = 0) const;     /* the object's own arrays: what Compute* writes */
    is_instance_buffers LastInstanceBuffers(int image) const;     /* what the consumers read (a sweep: its selected set) */
    /* the instance arrays of frame `image` of set `set` inside d_sweep_instances */
    is_instance_buffers SweepInstanceBuffers(int set, int image) const;
    size_t SweepInstanceStride() const;
    /* the Sections the consumers read: d_stixels, or the selected set of a sweep */
    const Section* LastSections() const;
    /* the Sections of `n_images` frames at `d_sections` to the host, as ComputeBatch delivers them */
    void FetchSections(const Section* d_sections, int n_images, const float* alpha, const int* vhor,
                       std::vector<StixelsData>& out, void* stream);
    /* the (column, section) -> label mappings of the frames whose instance arrays are ibs[0 .. n) */
    void FetchInstanceMappings(const std::vector<is_instance_buffers>& ibs, std::vector<InstanceMapping>& out,
                               void* stream);
    /* The last SweepBatch while it is what the consumers read (RememberBatch ends it). */
    struct Sweep {
        int sets = 0;      /* 0: the last compute call was not a sweep */
        int frames = 0;    /* frames per set */
        int selected = 0;
        bool instances = false;
    } m_sweep;
    /* The per-section instance map of frames 0 .. n_images-1 for RenderBatch, InstanceOverlapBatch and WorldBatch*:
     * the ground-truth map while it is active (nothing is launched), else the cluster labels of the last compute call
     * scattered into d_section_instance on `stream`; null after a call without instances. */
    const int32_t* SectionInstanceMap(int n_images, void* stream);
    bool HaveInstances() const { return m_last.gt_instances || m_last.cluster_instances; }
    /* What the last compute call left in d_stixels: the one record that RenderBatch, InstanceOverlapBatch, WorldBatch*,
     * AssignInstancesGTBatch and InstanceObjectsBatch* consume.  Two writers: RememberBatch (Compute, ComputeBatch) and
     * ForgetBatch (Finish, and ComputeBatchGather, which reuses d_stixels for its shard). */
    struct LastBatch {
        int frames = 0;                 /* 0: nothing to consume */
        bool cluster_instances = false; /* its cluster labels are in d_instance_labels */
        bool gt_instances = false;      /* the consumers read the ground-truth map (AssignInstancesGTBatch) */
        std::vector<float> alpha;       /* [frames] road parameters, library-convention vhor */
        std::vector<int> vhor;
        std::vector<int32_t> known_offsets; /* after a ComputeBatch: the sections in front of every frame, else empty */
    } m_last;
    void RememberBatch(int frames, bool cluster_instances, const float* alpha, const int* vhor);
    void ForgetBatch();
    /* How every consumer opens (a new one starts here): std::invalid_argument unless frames 0 .. n_images-1 of m_last
     * exist; then the caller's scope runs on the object's device, and a null `stream` becomes the object's own. */
    struct ConsumerScope;
    ConsumerScope BeginConsumer(const char* name, const char* verb, int n_images, void*& stream);
    /* what every consumer's args struct says alike: the Sections of frames first .. first + n_images - 1 and their
     * geometry (n_images, realcols, max_sections, rows, cols; is_world_args has no cols) */
    template <class Args> void FillGeometry(Args& a, int n_images, int first = 0) const;
    void FillGeometry(is_world_args& a, int n_images) const;
    /* the return code of a consumer's core call: IS_EINVAL is the caller's fault ("<name>: <the core's text>") */
    static void CheckConsumer(const char* name, int rc);
    GroundModel m_ground; /* per-frame ground model, storage reused between frames */
    /* the road parameters m_ground was computed for: a frame with the same parameters (a fixed
     * camera model, a replayed sequence) reuses it -- 1024 rows of erf / sqrt / log on the host
     * are 12 us of a 0.26 ms frame.  Invalidated by Initialize(). */
    float m_ground_key[12] = {0};  /* every input of PrecomputeGround */
    bool m_ground_valid = false;
    /* ComputeBatchRoad: the smallest library-convention horizon of the last batch, is_compute_road's vhor_min_hint for
     * the next one (-1: none yet) */
    int m_road_vhor_hint = -1;

    /* device (owned between Initialize and Finish, Stixels.cu:53-74, 136-163) */
    is_ctx* m_ctx = nullptr;
    Section* d_stixels = nullptr;             /* (aliases into d_stixels_block) */
    int32_t* d_instances_per_class = nullptr;
    int m_header_rows = 0;
    int m_head_sections = 0;
    /* AssignInstancesGTBatch: the parameters of the vote */
    double m_gt_min_fraction = 0.1;
    int m_gt_label_ids[IS_INSTANCE_CLASSES] = {24, 25, 26, 27, 28, 31, 32, 33};
    bool m_gt_is_train_ids = false;
    int m_overlap_capacity = 4096; /* records per frame of InstanceOverlapBatch's first pass */
    int m_world_capacity = 0;      /* records per frame of SetWorldCapacity; 0: not set */
    int m_idisp_capacity = 256;    /* keys per frame of ClusterInstanceDisparityBatch */
    /* SetSegmentationHead: weights | bias on the host, their K (0: not set), whether d_head_weights is behind them */
    std::vector<float> m_seghead_values;
    int m_seghead_K = 0;
    bool m_seghead_uploaded = false;
    int m_seghead_clamp_channel = -1;
    float m_seghead_clamp_lo = 0, m_seghead_clamp_hi = 0;
    /* InstanceObjectsBatch: objects per frame of the first pass, the capacities d_objects_block was laid out for */
    int m_object_capacity = 64;
    size_t m_objects_cap = 0, m_object_points_cap = 0;
    /* every device operation of the object runs on this stream (an ordinary stream: it still
     * synchronises with work the caller queued on the legacy NULL stream, like the reference's
     * default-stream code; on the NULL stream itself the auxiliary streams of the core never
     * overlap) */
    void* m_stream = nullptr;
    int m_max_batch = 1;
    int m_device = -1;      /* requested (SetDevice) */
    int m_ctx_device = -1;  /* resolved at Initialize(): where the buffers live */
    bool m_labels_on_host = false; /* h_instance_packed holds the triples of the last frame */

    StixelParameters m_params{};
    int m_max_sections = MAX_STIXELS_PER_COLUMN;
    bool m_is_initialized = false;

    /* probabilities */
    float m_pout = 0, m_pout_sky = 0;
    float m_pnexists_given_ground = 0, m_pnexists_given_object = 0, m_pnexists_given_sky = 0;
    float m_pord = 0, m_pgrav = 0, m_pblg = 0;
    /* camera */
    float m_focal = 0, m_baseline = 0, m_camera_tilt = 0, m_sigma_camera_tilt = 0;
    float m_camera_height = 0, m_sigma_camera_height = 0;
    float m_camera_center_x = -1, m_camera_center_y = -1;
    int m_vhor = 0;
    /* segmentation / weights */
    int m_segmentation_classes = 0, m_segmentation_channels = 0;
    float m_prior_weight = 0, m_disparity_weight = 0, m_segmentation_weight = 0,
          m_instance_weight = 0;
    /* disparity */
    int m_max_dis = 0;
    float m_max_disf = 0, m_invalid_disparity = -1;
    int m_rows = 0, m_cols = 0, m_realcols = 0;
    float m_sigma_disparity_object = 0, m_sigma_disparity_ground = 0, m_sigma_sky = 0;
    /* model */
    int m_column_step = 0;
    bool m_median_join = false;
    float m_alpha_ground = 0, m_range_objects_z = 0, m_epsilon = 0;
    int m_width_margin = 0;
    /* tables */
    std::vector<float> m_log_lut, m_obj_cost_lut, m_object_disparity_range;
    std::vector<float> m_normalization_object, m_inv_sigma2_object;
    float m_max_dis_log = 0, m_rows_log = 0;
    float m_puniform = 0, m_puniform_sky = 0, m_normalization_sky = 0, m_inv_sigma2_sky = 0;
    /* instances (host mirrors) */
    std::vector<int> m_instances_per_class;
    int m_instance_classes = IS_INSTANCE_CLASSES;
};

#endif
