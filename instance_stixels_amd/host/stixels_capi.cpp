/*
 * stixels_capi.cpp -- flat C view of the C++ `Stixels` host class, so that Python tests and
 * bench.py drive the SAME host code a C++ caller (run_cityscapes, StixelsWrapper) would:
 * SetConfig -> Initialize -> [SetDisparityImage, SetSegmentation, SetRoadParameters, Compute,
 * GetInstanceStixels] -> Finish  (call sequence of apps/run_cityscapes.cu:328-449).
 * C++ exceptions are turned into a negative return code + message.
 */
#include <algorithm>
#include <cstring>
#include <ctime>
#include <exception>
#include <stdexcept>
#include <string>
#include <vector>

#include "instance_stixels_core.h"
#include "is_numerics.h"
#include "InstanceStixels/RoadEstimation.h"
#include "InstanceStixels/Stixels.hpp"

namespace {
thread_local std::string g_host_err;
template <class F>
int guard(F&& f) {
    try {
        f();
        return 0;
    } catch (const std::invalid_argument& e) {
        g_host_err = e.what();
        return -1;
    } catch (const std::exception& e) {
        g_host_err = e.what();
        return -2;
    }
}
/* A result that stays with the calling thread between the call that computed it for object `h` and the one call that
 * copies it out: set for h, taken once by h if it fits the caller's arrays (else refused, and kept), cleared. */
template <class T>
struct Pending {
    T value{};
    void* owner = nullptr;
    void clear() { set(nullptr, T()); }
    void set(void* h, T v) { value = std::move(v), owner = h; }
    const T& take(void* h, bool fits, const char* refusal) {
        if (h != owner || !fits) throw std::invalid_argument(refusal);
        owner = nullptr;
        return value;
    }
};
struct WorldRecords { const is_world_stixel* records; int64_t n; };
thread_local Pending<std::vector<is_overlap_record>> g_overlap;
thread_local Pending<WorldRecords> g_world;
thread_local Pending<Stixels::InstanceObjectsView> g_objects;
thread_local Pending<std::vector<int32_t>> g_gt_quads;

/* road [n][4] = (vhor_image, camera_tilt, camera_height, alpha_ground) */
Stixels::RoadParameters road_record(const float* r) { return Stixels::RoadParameters{(int)r[0], r[1], r[2], r[3]}; }
std::vector<Stixels::RoadParameters> to_road(const float* road, int n) {
    std::vector<Stixels::RoadParameters> rp(n);
    for (int i = 0; i < n; i++) rp[i] = road_record(road + 4 * i);
    return rp;
}
}  // namespace

extern "C" {

/* C mirror of StixelConfig (types.h), field for field. */
struct ish_config {
    float rows, cols;
    int max_dis;
    float invalid_disparity, eps;
    int min_pts, size_filter, n_semantic_classes, n_offset_channels;
    float prior_weight, segmentation_weight, instance_weight, disparity_weight;
    int pairwise, column_step;
    float focal, baseline, camera_center_x, camera_center_y;
    float sigma_disparity_object, sigma_disparity_ground, sigma_sky;
    float pout, pout_sky, pord, pgrav, pblg;
    float pground_given_nexist, pobject_given_nexist, psky_given_nexist, pnexist_dis;
    float pground, pobject, psky;
    int width_margin;
    float sigma_camera_tilt, sigma_camera_height;
    int median_join;
    float epsilon, range_objects_z, road_vdisparity_threshold;
};

static StixelConfig to_cpp(const ish_config* c) {
    StixelConfig s;
    s.rows = c->rows; s.cols = c->cols; s.max_dis = c->max_dis;
    s.invalid_disparity = c->invalid_disparity; s.eps = c->eps; s.min_pts = c->min_pts;
    s.size_filter = c->size_filter; s.n_semantic_classes = c->n_semantic_classes;
    s.n_offset_channels = c->n_offset_channels; s.prior_weight = c->prior_weight;
    s.segmentation_weight = c->segmentation_weight; s.instance_weight = c->instance_weight;
    s.disparity_weight = c->disparity_weight; s.pairwise = c->pairwise != 0;
    s.column_step = c->column_step; s.focal = c->focal; s.baseline = c->baseline;
    s.camera_center_x = c->camera_center_x; s.camera_center_y = c->camera_center_y;
    s.sigma_disparity_object = c->sigma_disparity_object;
    s.sigma_disparity_ground = c->sigma_disparity_ground; s.sigma_sky = c->sigma_sky;
    s.pout = c->pout; s.pout_sky = c->pout_sky; s.pord = c->pord; s.pgrav = c->pgrav;
    s.pblg = c->pblg; s.pground_given_nexist = c->pground_given_nexist;
    s.pobject_given_nexist = c->pobject_given_nexist;
    s.psky_given_nexist = c->psky_given_nexist; s.pnexist_dis = c->pnexist_dis;
    s.pground = c->pground; s.pobject = c->pobject; s.psky = c->psky;
    s.width_margin = c->width_margin; s.sigma_camera_tilt = c->sigma_camera_tilt;
    s.sigma_camera_height = c->sigma_camera_height; s.median_join = c->median_join != 0;
    s.epsilon = c->epsilon; s.range_objects_z = c->range_objects_z;
    s.road_vdisparity_threshold = c->road_vdisparity_threshold;
    return s;
}

const char* ish_last_error(void) { return g_host_err.c_str(); }

void* ish_create(void) { return new Stixels(); }
void ish_destroy(void* h) { delete (Stixels*)h; }

int ish_set_config(void* h, const ish_config* c) {
    return guard([&] { ((Stixels*)h)->SetConfig(to_cpp(c)); });
}
int ish_initialize(void* h, int max_batch) {
    return guard([&] { ((Stixels*)h)->InitializeBatch(max_batch); });
}
int ish_precompute_host(void* h) {
    return guard([&] { ((Stixels*)h)->PrecomputeHost(); });
}
int ish_finish(void* h) {
    return guard([&] {
        if (((Stixels*)h)->IsInitialized()) ((Stixels*)h)->Finish();
    });
}
int ish_is_initialized(void* h) { return ((Stixels*)h)->IsInitialized() ? 1 : 0; }
int ish_real_cols(void* h) { return ((Stixels*)h)->GetRealCols(); }
int ish_max_sections(void* h) { return ((Stixels*)h)->GetMaxSections(); }

int ish_get_parameters(void* h, StixelParameters* out) {
    *out = ((Stixels*)h)->GetParameters();
    return 0;
}
int ish_get_luts(void* h, float* obj_cost_lut, float* obj_disparity_range) {
    Stixels* s = (Stixels*)h;
    std::memcpy(obj_cost_lut, s->GetObjectCostLUT().data(),
                s->GetObjectCostLUT().size() * sizeof(float));
    std::memcpy(obj_disparity_range, s->GetObjectDisparityRange().data(),
                s->GetObjectDisparityRange().size() * sizeof(float));
    return 0;
}
void* ish_core_context(void* h) { return ((Stixels*)h)->GetCoreContext(); }

int ish_set_disparity_image(void* h, const float* data, size_t n) {
    return guard([&] { ((Stixels*)h)->SetDisparityImage(std::vector<pixel_t>(data, data + n)); });
}
int ish_set_segmentation(void* h, const int32_t* data, size_t n) {
    return guard([&] { ((Stixels*)h)->SetSegmentation(std::vector<int32_t>(data, data + n)); });
}
int ish_set_road_parameters(void* h, int vhor, float tilt, float height, float alpha) {
    return guard([&] { ((Stixels*)h)->SetRoadParameters(vhor, tilt, height, alpha); });
}
int ish_get_ground_model(void* h, float* gf, float* ng, float* ig, int* vhor_lib) {
    return guard([&] {
        std::vector<float> a, b, c;
        ((Stixels*)h)->GetGroundModel(a, b, c, *vhor_lib);
        std::memcpy(gf, a.data(), a.size() * sizeof(float));
        std::memcpy(ng, b.data(), b.size() * sizeof(float));
        std::memcpy(ig, c.data(), c.size() * sizeof(float));
    });
}

/* Compute(): sections [realcols*max_sections]; header fields through `hdr[9]` =
 * rows, cols, realcols, max_sections, max_dis, column_step, semantic_classes, vhor, (unused). */
int ish_compute(void* h, int pairwise, Section* sections, int* hdr, float* alpha_ground,
                float* ret) {
    return guard([&] {
        StixelsData d;
        *ret = ((Stixels*)h)->Compute(pairwise != 0, d);
        std::memcpy(sections, d.sections.data(), d.sections.size() * sizeof(Section));
        hdr[0] = d.rows; hdr[1] = d.cols; hdr[2] = d.realcols; hdr[3] = d.max_sections;
        hdr[4] = d.max_dis; hdr[5] = d.column_step; hdr[6] = d.semantic_classes; hdr[7] = d.vhor;
        *alpha_ground = d.alpha_ground;
    });
}

/* Times n_iter calls of Stixels::Compute() on the frame set before (SetDisparityImage /
 * SetSegmentation / SetRoadParameters), StixelsData reused like a C++ caller's loop would; with
 * `with_instances` every frame also fetches GetInstanceStixels().  -> seconds per frame. */
int ish_time_compute(void* h, int pairwise, int n_iter, int with_instances, double* s_per_frame) {
    return guard([&] {
        Stixels* s = (Stixels*)h;
        StixelsData d;
        for (int i = 0; i < 3; i++) s->Compute(pairwise != 0, d);
        timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        size_t sink = 0;
        for (int i = 0; i < n_iter; i++) {
            s->Compute(pairwise != 0, d);
            if (with_instances) sink += s->GetInstanceStixels().size();
        }
        clock_gettime(CLOCK_MONOTONIC, &t1);
        (void)sink;
        *s_per_frame = ((t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec)) / n_iter;
    });
}

/* ComputeBatch() on device-resident inputs.  road: [n][4] = (vhor_image, camera_tilt,
 * camera_height, alpha_ground); sections: [n][realcols*max_sections]; vhor_lib: [n].
 * triples (optional): [n][cap][3] (column, section, label) of every frame, counts: [n]. */
int ish_compute_batch(void* h, int pairwise, int n_images, const float* d_big, const int32_t* d_seg,
                      const float* road, Section* sections, int* vhor_lib, int* triples, int cap,
                      int* counts, void* stream) {
    return guard([&] {
        Stixels* s = (Stixels*)h;
        const std::vector<Stixels::RoadParameters> rp = to_road(road, n_images);
        std::vector<StixelsData> out;
        std::vector<Stixels::InstanceMapping> maps;
        s->ComputeBatch(pairwise != 0, n_images, d_big, d_seg, rp.data(), out, stream,
                        triples ? &maps : nullptr);
        for (int i = 0; i < n_images; i++) {
            std::memcpy(sections + (size_t)i * out[i].sections.size(), out[i].sections.data(),
                        out[i].sections.size() * sizeof(Section));
            vhor_lib[i] = out[i].vhor;
            if (triples) {
                int n = 0;
                for (const auto& kv : maps[i]) {
                    if (n >= cap) break;
                    int* t = triples + ((size_t)i * cap + n) * 3;
                    t[0] = kv.first.first; t[1] = kv.first.second; t[2] = kv.second;
                    n++;
                }
                counts[i] = (int)maps[i].size();
            }
        }
    });
}

/* ComputeBatchGather(): this rank's shard + the RCCL gather of every rank's Sections on `dst`.
 * road: [n][4] of this rank; images_per_rank: [ranks]; road_all: [sum][4] (dst only, else null);
 * sections_all: [sum][realcols*max_sections] on dst; *n_out: frames written (0 on the other ranks). */
int ish_compute_batch_gather(void* h, int pairwise, int n_images, const float* d_big, const int32_t* d_seg,
                             const float* road, void* comm, int dst, const int* images_per_rank,
                             const float* road_all, int n_all, Section* sections_all, int* vhor_all,
                             int* n_out, void* stream) {
    return guard([&] {
        Stixels* s = (Stixels*)h;
        if (road_all) { /* dst: the caller sized road_all / sections_all / vhor_all for n_all frames */
            int rank = 0, nranks = 0;
            if (is_comm_rank(comm, &rank, &nranks) != IS_OK)
                throw std::runtime_error(std::string("ish_compute_batch_gather: ") + is_last_error());
            long sum = 0;
            for (int r = 0; r < nranks; r++) sum += images_per_rank[r];
            if (sum != (long)n_all)
                throw std::invalid_argument("ish_compute_batch_gather: n_all differs from the sum of images_per_rank");
        }
        const std::vector<Stixels::RoadParameters> rp = to_road(road, n_images);
        const std::vector<Stixels::RoadParameters> ra = road_all ? to_road(road_all, n_all)
                                                                 : std::vector<Stixels::RoadParameters>();
        std::vector<StixelsData> out;
        s->ComputeBatchGather(pairwise != 0, n_images, d_big, d_seg, rp.data(), comm, dst, images_per_rank,
                              road_all ? ra.data() : nullptr, out, stream);
        *n_out = (int)out.size();
        for (size_t i = 0; i < out.size() && i < (size_t)(n_all > 0 ? n_all : 0); i++) {
            std::memcpy(sections_all + i * out[i].sections.size(), out[i].sections.data(),
                        out[i].sections.size() * sizeof(Section));
            vhor_all[i] = out[i].vhor;
        }
    });
}

/* Times n_iter ComputeBatch() calls of n_images frames (inputs resident on the device), with or
 * without the per-frame instance mappings.  -> seconds per call. */
int ish_time_compute_batch(void* h, int pairwise, int n_images, const float* d_big, const int32_t* d_seg,
                           const float* road, int n_iter, int with_instances, double* s_per_call) {
    return guard([&] {
        Stixels* s = (Stixels*)h;
        const std::vector<Stixels::RoadParameters> rp = to_road(road, n_images);
        std::vector<StixelsData> out;
        std::vector<Stixels::InstanceMapping> maps;
        s->ComputeBatch(pairwise != 0, n_images, d_big, d_seg, rp.data(), out, nullptr,
                        with_instances ? &maps : nullptr);
        timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        for (int i = 0; i < n_iter; i++)
            s->ComputeBatch(pairwise != 0, n_images, d_big, d_seg, rp.data(), out, nullptr,
                            with_instances ? &maps : nullptr);
        clock_gettime(CLOCK_MONOTONIC, &t1);
        *s_per_call = ((t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec)) / n_iter;
    });
}

/* RenderBatch(): frames 0 .. n-1 of the last Compute() / ComputeBatch() to dense maps + scores (every device
 * pointer optional; class_to_label: host [n_classes] or null for Cityscapes).  disp_abs_sum / disp_count /
 * stixel_count: host [n] each. */
int ish_render_batch(void* h, int n, uint8_t* label, float* disparity, int32_t* instance, const uint8_t* gt_label,
                     int n_labels, unsigned long long* confusion, const float* gt_disparity,
                     const uint8_t* class_to_label, int n_classes, double* disp_abs_sum, int64_t* disp_count,
                     int32_t* stixel_count, void* stream) {
    return guard([&] {
        Stixels::RenderTargets t;
        t.label = label; t.disparity = disparity; t.instance = instance;
        t.gt_label = gt_label; t.n_labels = n_labels; t.confusion = confusion; t.gt_disparity = gt_disparity;
        t.class_to_label = class_to_label; t.n_classes = n_classes;
        const std::vector<Stixels::RenderResult> r = ((Stixels*)h)->RenderBatch(n, t, stream);
        for (int i = 0; i < n; i++) {
            disp_abs_sum[i] = r[i].disp_abs_sum;
            disp_count[i] = r[i].disp_count;
            stixel_count[i] = r[i].stixel_count;
        }
    });
}

/* InstanceOverlapBatch(): the tables of frames 0 .. n-1 of the last Compute() / ComputeBatch() against
 * d_gt_instance.  n_records: host [n].  The records stay with the calling thread until ish_instance_overlap_records
 * copies them out (all frames back to back, in frame order) -- the caller sizes that buffer from n_records. */
int ish_instance_overlap_batch(void* h, int n, const int32_t* d_gt_instance, int64_t* n_records, void* stream) {
    return guard([&] {
        g_overlap.clear();
        const std::vector<std::vector<is_overlap_record>> t = ((Stixels*)h)->InstanceOverlapBatch(n, d_gt_instance,
                                                                                                  stream);
        std::vector<is_overlap_record> all;
        for (int i = 0; i < n; i++) {
            n_records[i] = (int64_t)t[i].size();
            all.insert(all.end(), t[i].begin(), t[i].end());
        }
        g_overlap.set(h, std::move(all));
    });
}
int ish_instance_overlap_records(void* h, is_overlap_record* out, int64_t cap) {
    return guard([&] {
        const std::vector<is_overlap_record>& t = g_overlap.take(
            h, (int64_t)g_overlap.value.size() <= cap,
            "ish_instance_overlap_records: no tables of this object, or cap too small.");
        std::memcpy(out, t.data(), t.size() * sizeof(is_overlap_record));
    });
}
int ish_set_instance_overlap_capacity(void* h, int records) {
    return guard([&] { ((Stixels*)h)->SetInstanceOverlapCapacity(records); });
}

/* WorldBatch(): the records of frames 0 .. n-1 of the last Compute() / ComputeBatch().  frame_offsets: host
 * [n + 1].  The records stay in the object's pinned buffer (Stixels::WorldBatchView) until ish_world_records copies
 * them into the caller's array (cap in records, sized from frame_offsets[n]; an array the caller keeps from batch to
 * batch costs no fresh pages): ONE copy on the host.  Both calls from the same thread, nothing of this object in
 * between. */
int ish_world_batch(void* h, int n, int32_t* frame_offsets, void* stream) {
    return guard([&] {
        g_world.clear();
        std::vector<int32_t> offsets;
        const is_world_stixel* records = ((Stixels*)h)->WorldBatchView(n, offsets, stream);
        std::memcpy(frame_offsets, offsets.data(), offsets.size() * sizeof(int32_t));
        g_world.set(h, WorldRecords{records, offsets[n]});
    });
}
int ish_world_records(void* h, is_world_stixel* out, int64_t cap) {
    return guard([&] {
        const WorldRecords& w = g_world.take(h, g_world.value.n <= cap,
                                             "ish_world_records: no records of this object, or cap too small.");
        Stixels::CopyWorldRecords(out, w.records, (size_t)w.n);
    });
}
int ish_set_world_capacity(void* h, int records_per_frame) {
    return guard([&] { ((Stixels*)h)->SetWorldCapacity(records_per_frame); });
}

/* InstanceObjectsBatch(): the per-instance objects and contour points of frames 0 .. n-1 of the last Compute() /
 * ComputeBatch().  frame_objects, frame_points: host [n]; totals: host [2] (objects, points).  The records stay in
 * the object's pinned buffer (Stixels::InstanceObjectsBatchView) until ish_instance_objects_records copies them into
 * the caller's arrays (capacities in records, sized from totals).  Both calls from the same thread, nothing of this
 * object in between. */
int ish_instance_objects_batch(void* h, int n, int32_t* frame_objects, int32_t* frame_points, int32_t* totals,
                               void* stream) {
    return guard([&] {
        g_objects.clear();
        const Stixels::InstanceObjectsView v = ((Stixels*)h)->InstanceObjectsBatchView(n, stream);
        std::memcpy(frame_objects, v.frame_objects, n * sizeof(int32_t));
        std::memcpy(frame_points, v.frame_points, n * sizeof(int32_t));
        totals[0] = v.n_objects;
        totals[1] = v.n_points;
        g_objects.set(h, v);
    });
}
int ish_instance_objects_records(void* h, is_instance_object* objects, int64_t cap_objects, is_contour_point* points,
                                 int64_t cap_points) {
    return guard([&] {
        const Stixels::InstanceObjectsView& v = g_objects.take(
            h, g_objects.value.n_objects <= cap_objects && g_objects.value.n_points <= cap_points,
            "ish_instance_objects_records: no records of this object, or cap too small.");
        if (v.n_objects) std::memcpy(objects, v.objects, (size_t)v.n_objects * sizeof(is_instance_object));
        if (v.n_points) std::memcpy(points, v.points, (size_t)v.n_points * sizeof(is_contour_point));
    });
}
int ish_set_instance_object_capacity(void* h, int objects_per_frame) {
    return guard([&] { ((Stixels*)h)->SetInstanceObjectCapacity(objects_per_frame); });
}

/* AssignInstancesGTBatch(): the ground-truth vote over frames 0 .. n-1 of the last Compute() / ComputeBatch(); from
 * then on RenderBatch / InstanceOverlapBatch / WorldBatch read its map.  n_quads (optional): the number of labelled
 * sections; their (frame, column, section, label) quads stay with the calling thread until ish_assign_instances_gt_quads
 * copies them out -- the caller sizes that buffer from *n_quads.  Null: no mapping is fetched, the call is asynchronous. */
int ish_assign_instances_gt_batch(void* h, int n, const int32_t* d_gt_instance, int64_t* n_quads, void* stream) {
    return guard([&] {
        g_gt_quads.clear();
        std::vector<Stixels::InstanceMapping> maps;
        ((Stixels*)h)->AssignInstancesGTBatch(n, d_gt_instance, stream, n_quads ? &maps : nullptr);
        if (!n_quads) return;
        std::vector<int32_t> quads;
        for (int i = 0; i < n; i++)
            for (const auto& kv : maps[i]) {
                const int32_t q[4] = {i, kv.first.first, kv.first.second, kv.second};
                quads.insert(quads.end(), q, q + 4);
            }
        *n_quads = (int64_t)(quads.size() / 4);
        g_gt_quads.set(h, std::move(quads));
    });
}
int ish_assign_instances_gt_quads(void* h, int32_t* out, int64_t cap) {
    return guard([&] {
        const std::vector<int32_t>& q = g_gt_quads.take(
            h, (int64_t)(g_gt_quads.value.size() / 4) <= cap,
            "ish_assign_instances_gt_quads: no quads of this object, or cap too small.");
        if (!q.empty()) std::memcpy(out, q.data(), q.size() * sizeof(int32_t));
    });
}
/* GroundTruthOffsetsBatch(): channels 19 and 20 of d_segmentation from the ground truth; asynchronous on `stream`. */
int ish_ground_truth_offsets_batch(void* h, int n, const int32_t* d_gt_instance, int32_t* d_segmentation,
                                   void* stream) {
    return guard([&] { ((Stixels*)h)->GroundTruthOffsetsBatch(n, d_gt_instance, d_segmentation, stream); });
}
/* SetSegmentationHead(): weight [channels][K], bias [channels] host floats.  Needs no device. */
int ish_set_segmentation_head(void* h, const float* weight, size_t n_weight, const float* bias, size_t n_bias, int K) {
    return guard([&] {
        if ((n_weight && !weight) || (n_bias && !bias)) throw std::invalid_argument("SetSegmentationHead: null array.");
        ((Stixels*)h)->SetSegmentationHead(std::vector<float>(weight, weight + n_weight),
                                           std::vector<float>(bias, bias + n_bias), K);
    });
}
int ish_set_segmentation_head_clamp(void* h, int channel, float lo, float hi) {
    return guard([&] { ((Stixels*)h)->SetSegmentationHeadClamp(channel, lo, hi); });
}
/* SegmentationHeadBatch(): backbone features -> d_segmentation (and d_cnn_out, may be null); asynchronous on `stream`. */
int ish_segmentation_head_batch(void* h, int n, const void* d_features, int dtype, int32_t* d_segmentation,
                                float* d_cnn_out, void* stream) {
    return guard([&] { ((Stixels*)h)->SegmentationHeadBatch(n, d_features, dtype, d_segmentation, d_cnn_out, stream); });
}
/* CnnLabelBatch(): the head's float output -> the CNN's label image, cell classes and confusion table (each may be
 * null; gt_label and confusion go together); asynchronous on `stream`. */
int ish_cnn_label_batch(void* h, int n, const float* d_cnn_out, int mode, uint8_t* d_class8, uint8_t* d_label,
                        const uint8_t* d_gt_label, int n_labels, unsigned long long* d_confusion, void* stream) {
    return guard([&] {
        Stixels::CnnLabelTargets t;
        t.class8 = d_class8;
        t.label = d_label;
        t.gt_label = d_gt_label;
        t.n_labels = n_labels;
        t.confusion = d_confusion;
        ((Stixels*)h)->CnnLabelBatch(n, d_cnn_out, mode, t, stream);
    });
}
int ish_use_cluster_instances(void* h) {
    return guard([&] { ((Stixels*)h)->UseClusterInstances(); });
}
/* label_ids8: host [8] or null for Cityscapes */
int ish_set_gt_assignment_parameters(void* h, double min_fraction, const int* label_ids8, int gt_is_train_ids) {
    return guard([&] { ((Stixels*)h)->SetGTAssignmentParameters(min_fraction, label_ids8, gt_is_train_ids != 0); });
}

/* ---- parameter sweeps.  sets: [n_sets][7] floats = (prior, disparity, segmentation, instance weight, eps, min_pts,
 * size_filter), the weights in SetWeightParameters' user-facing form.  min_pts and size_filter travel as float32:
 * exact up to 2^24, far above any number of sections or rows. ---- */
static std::vector<Stixels::SweepSet> to_sets(const float* sets, int n) {
    std::vector<Stixels::SweepSet> v((size_t)std::max(n, 0));
    for (int k = 0; k < n; k++) {
        const float* s = sets + 7 * (size_t)k;
        v[k] = Stixels::SweepSet{s[0], s[1], s[2], s[3], s[4], (int)s[5], (int)s[6]};
    }
    return v;
}
static void copy_maps(const std::vector<Stixels::InstanceMapping>& maps, int* triples, int cap, int* counts) {
    for (size_t i = 0; i < maps.size(); i++) {
        int n = 0;
        for (const auto& kv : maps[i]) {
            if (n >= cap) break;
            int* t = triples + (i * (size_t)cap + n) * 3;
            t[0] = kv.first.first; t[1] = kv.first.second; t[2] = kv.second;
            n++;
        }
        counts[i] = (int)maps[i].size();
    }
}
/* Stixels::CoreSweepSet: needs no device */
int ish_core_sweep_set(const float* set7, is_sweep_set* out) {
    return guard([&] { *out = Stixels::CoreSweepSet(to_sets(set7, 1)[0]); });
}
int ish_sweep_batch(void* h, int pairwise, int n_images, const float* d_big, const int32_t* d_seg, const float* road,
                    const float* sets, int n_sets, int with_instances, void* stream) {
    return guard([&] {
        const std::vector<Stixels::RoadParameters> rp = to_road(road, n_images > 0 ? n_images : 0);
        ((Stixels*)h)->SweepBatch(pairwise != 0, n_images, d_big, d_seg, rp.data(), to_sets(sets, n_sets), stream,
                                  with_instances != 0);
    });
}
int ish_select_sweep_set(void* h, int k) {
    return guard([&] { ((Stixels*)h)->SelectSweepSet(k); });
}
/* frames of the last compute call the consumers can read; sets of the last sweep (0: not a sweep); the device of
 * the object's buffers (-1 before Initialize); each < -1 on a null handle */
static int handle_query(void* h, int (*f)(Stixels*)) {
    int v = 0;
    const int rc = guard([&] {
        if (!h) throw std::invalid_argument("null handle");
        v = f((Stixels*)h);
    });
    return rc ? rc - 1 : v;
}
int ish_last_frames(void* h) { return handle_query(h, [](Stixels* s) { return s->LastFrames(); }); }
int ish_sweep_sets(void* h) { return handle_query(h, [](Stixels* s) { return s->SweepSets(); }); }
int ish_active_device(void* h) { return handle_query(h, [](Stixels* s) { return s->GetActiveDevice(); }); }
/* SweepSections(k): sections [frames][realcols*max_sections], vhor_lib and alpha_ground [frames]; triples (optional):
 * [frames][cap][3], counts [frames], as ish_compute_batch */
int ish_sweep_sections(void* h, int k, Section* sections, int* vhor_lib, float* alpha_ground, int* triples, int cap,
                       int* counts) {
    return guard([&] {
        std::vector<StixelsData> out;
        std::vector<Stixels::InstanceMapping> maps;
        ((Stixels*)h)->SweepSections(k, out, triples ? &maps : nullptr);
        for (size_t i = 0; i < out.size(); i++) {
            std::memcpy(sections + i * out[i].sections.size(), out[i].sections.data(),
                        out[i].sections.size() * sizeof(Section));
            vhor_lib[i] = out[i].vhor;
            alpha_ground[i] = out[i].alpha_ground;
        }
        if (triples) copy_maps(maps, triples, cap, counts);
    });
}
/* ReclusterBatch(): triples (optional): [n_frames][cap][3], counts [n_frames], n_frames = ish_last_frames() */
int ish_recluster_batch(void* h, float eps, int min_pts, int size_filter, int n_frames, int* triples, int cap, int* counts,
                        void* stream) {
    return guard([&] {
        Stixels* s = (Stixels*)h;
        if (triples && n_frames != s->LastFrames())
            throw std::invalid_argument("ish_recluster_batch: n_frames differs from the frames of the last compute call");
        std::vector<Stixels::InstanceMapping> maps;
        s->ReclusterBatch(eps, min_pts, size_filter, triples ? &maps : nullptr, stream);
        if (triples) copy_maps(maps, triples, cap, counts);
    });
}

/* ClusterInstanceDisparityBatch(): gt_instance / disparity_u8 device arrays, or host arrays with inputs_on_host;
 * triples (optional): [n][cap][3], counts [n]; stixel_median (optional): host [n][realcols][max_sections] */
int ish_cluster_instance_disparity_batch(void* h, int n, const int32_t* gt_instance, const uint8_t* disparity_u8,
                                         int inputs_on_host, float eps, int min_pts, int size_filter, int* triples,
                                         int cap, int* counts, float* stixel_median, void* stream) {
    return guard([&] {
        std::vector<Stixels::InstanceMapping> maps;
        ((Stixels*)h)->ClusterInstanceDisparityBatch(n, gt_instance, disparity_u8, eps, min_pts, size_filter,
                                                     triples ? &maps : nullptr, stixel_median, stream,
                                                     inputs_on_host != 0);
        if (triples) copy_maps(maps, triples, cap, counts);
    });
}
int ish_set_instance_disparity_capacity(void* h, int keys_per_frame) {
    return guard([&] { ((Stixels*)h)->SetInstanceDisparityCapacity(keys_per_frame); });
}

int ish_set_device(void* h, int device) {
    return guard([&] { ((Stixels*)h)->SetDevice(device); });
}

/* GetInstanceStixels(): triples (column, section, label); returns the count (<= cap) or <0. */
int ish_get_instance_stixels(void* h, int* triples, int cap) {
    int n = 0;
    const int rc = guard([&] {
        const auto m = ((Stixels*)h)->GetInstanceStixels();
        for (const auto& kv : m) {
            if (n >= cap) break;
            triples[3 * n] = kv.first.first;
            triples[3 * n + 1] = kv.first.second;
            triples[3 * n + 2] = kv.second;
            n++;
        }
    });
    return rc ? rc : n;
}

int ish_get_3d_vertices(void* h, const Section* sections, float alpha_ground, int vhor,
                        float* out, int cap) {
    int n = 0;
    const int rc = guard([&] {
        Stixels* s = (Stixels*)h;
        StixelsData d;
        d.sections.assign(sections, sections + (size_t)s->GetRealCols() * s->GetMaxSections());
        d.alpha_ground = alpha_ground;
        d.vhor = vhor;
        const std::vector<float> v = s->Get3DVertices(d);
        n = (int)std::min<size_t>(v.size(), (size_t)cap);
        std::memcpy(out, v.data(), (size_t)n * sizeof(float));
    });
    return rc ? rc : n;
}

int ish_save_stixels(void* h, Section* sections, const int* triples, int n_triples,
                     float alpha_ground, int vhor, const char* fname) {
    return guard([&] {
        Stixels* s = (Stixels*)h;
        std::map<std::pair<int, int>, int> m;
        for (int i = 0; i < n_triples; i++)
            m[std::make_pair(triples[3 * i], triples[3 * i + 1])] = triples[3 * i + 2];
        Stixels::SaveStixels(sections, m, alpha_ground, vhor, s->GetRealCols(),
                             s->GetMaxSections(), fname);
    });
}

/* ---- RoadEstimation (f3) ---- */
void* ire_create(void) { return new RoadEstimation(); }
void ire_destroy(void* h) { delete (RoadEstimation*)h; }
int ire_initialize(void* h, float cy, float baseline, float focal, int rows, int cols, int max_dis,
                   float threshold) {
    return guard([&] { ((RoadEstimation*)h)->Initialize(cy, baseline, focal, rows, cols, max_dis, threshold); });
}
int ire_finish(void* h) {
    return guard([&] {
        if (((RoadEstimation*)h)->IsInitialized()) ((RoadEstimation*)h)->Finish();
    });
}
/* returns 1 if a road line was found; out = pitch, camera height, slope, horizon point */
int ire_compute(void* h, const float* image, size_t n, float* out4) {
    int ok = 0;
    const int rc = guard([&] {
        RoadEstimation* r = (RoadEstimation*)h;
        ok = r->Compute(std::vector<pixel_t>(image, image + n)) ? 1 : 0;
        out4[0] = r->GetPitch(); out4[1] = r->GetCameraHeight(); out4[2] = r->GetSlope();
        out4[3] = (float)r->GetHorizonPoint();
    });
    return rc ? rc : ok;
}
int ire_set_device(void* h, int device) {
    return guard([&] { ((RoadEstimation*)h)->SetDevice(device); });
}
int ire_active_device(void* h) { return ((RoadEstimation*)h)->GetActiveDevice(); }
/* Compute(pixel_t* d_im): the disparity image is on the device already -- what the wrapper passes
 * after Stixels::GetInputDisparityImageOnDevice() (apps/stixels_wrapper.cu:187) */
int ire_compute_device(void* h, float* d_image, float* out4) {
    int ok = 0;
    const int rc = guard([&] {
        RoadEstimation* r = (RoadEstimation*)h;
        ok = r->Compute(d_image) ? 1 : 0;
        out4[0] = r->GetPitch(); out4[1] = r->GetCameraHeight(); out4[2] = r->GetSlope();
        out4[3] = (float)r->GetHorizonPoint();
    });
    return rc ? rc : ok;
}
/* ComputeBatch(d_disparity [n][rows][cols], n): out [n] Stixels::RoadParameters (int vhor, float tilt,
 * float height, float alpha: 16 bytes each), ok [n] uint8; stream: a hipStream_t or null (the object's own).
 * Returns the number of frames finished with the host Hough transform (GetBatchFallbacks()). */
static_assert(sizeof(Stixels::RoadParameters) == 16, "ire_compute_batch writes 16-byte records");
int ire_compute_batch(void* h, const float* d_disparity, int n, void* out, uint8_t* ok, void* stream) {
    const int rc = guard([&] {
        ((RoadEstimation*)h)->ComputeBatch(d_disparity, n, (Stixels::RoadParameters*)out, ok, stream);
    });
    return rc ? rc : ((RoadEstimation*)h)->GetBatchFallbacks();
}
int ire_set_batch_limits(void* h, int max_lines, int max_candidates) {
    return guard([&] { ((RoadEstimation*)h)->SetBatchLimits(max_lines, max_candidates); });
}
int ire_batch_fallbacks(void* h) { return h ? ((RoadEstimation*)h)->GetBatchFallbacks() : -1; }
void* ish_get_input_disparity_on_device(void* h) {
    return (void*)((Stixels*)h)->GetInputDisparityImageOnDevice();
}
int ire_get_binary(void* h, uint8_t* out, size_t n) {
    const auto& v = ((RoadEstimation*)h)->GetBinaryVDisparity();
    std::memcpy(out, v.data(), std::min(n, v.size()));
    return 0;
}
int ire_hough_lines(const uint8_t* image, int rows, int cols, float rho, float theta, int threshold,
                    float* out, int cap) {
    const auto lines = RoadEstimation::HoughLines(image, rows, cols, rho, theta, threshold);
    const int n = (int)std::min<size_t>(lines.size(), (size_t)cap);
    for (int i = 0; i < n; i++) { out[2 * i] = lines[i].first; out[2 * i + 1] = lines[i].second; }
    return (int)lines.size();
}
/* RoadEstimation::ChooseLine on lines [n][2] (rho, theta), without a device: the index of the accepted line
 * (out: one Stixels::RoadParameters record) or -1 (out untouched) */
int ire_choose_line(float cy, float baseline, float focal, int rows, const float* lines, int n, void* out) {
    std::vector<std::pair<float, float>> l((size_t)std::max(n, 0));
    for (int i = 0; i < n; i++) l[i] = std::make_pair(lines[2 * i], lines[2 * i + 1]);
    return RoadEstimation::ChooseLine(cy, baseline, focal, rows, l.data(), l.size(), *(Stixels::RoadParameters*)out);
}

/* ---- the device-resident road chain: the shared numerics and the host twins, for tests and callers ---- */
float ish_erff(float x) { return is_erff(x); }
float ish_atanf(float x) { return is_atanf(x); }
float ish_cosf(float x) { return is_cosf(x); }
void ish_erff_n(const float* x, float* out, size_t n) { for (size_t i = 0; i < n; i++) out[i] = is_erff(x[i]); }
void ish_atanf_n(const float* x, float* out, size_t n) { for (size_t i = 0; i < n; i++) out[i] = is_atanf(x[i]); }
void ish_cosf_n(const float* x, float* out, size_t n) { for (size_t i = 0; i < n; i++) out[i] = is_cosf(x[i]); }

/* Stixels::PrecomputeGroundShared with the object's constants and FastLog table (after PrecomputeHost() or
 * Initialize()): gf / ng / ig [rows], range_index [rows] or null */
int ish_precompute_ground_shared(void* h, int vhor_lib, float tilt, float height, float alpha, float* gf, float* ng,
                                 float* ig, int* range_index) {
    return guard([&] {
        Stixels* s = (Stixels*)h;
        const std::vector<float>& lut = s->GetLogLUT();
        if (lut.empty()) throw std::invalid_argument("ish_precompute_ground_shared before PrecomputeHost()");
        Stixels::PrecomputeGroundShared(s->GroundParams(), lut.data(), (int)lut.size(), s->GetParameters().rows,
                                        vhor_lib, tilt, height, alpha, gf, ng, ig, range_index);
    });
}
int ish_ground_params(void* h, is_ground_params* out) {
    return guard([&] { *out = ((Stixels*)h)->GroundParams(); });
}
/* the object's FastLog table: returns its entries; copies min(cap, entries) of them when out is not null */
int ish_log_lut(void* h, float* out, int cap) {
    const std::vector<float>& lut = ((Stixels*)h)->GetLogLUT();
    if (out) std::memcpy(out, lut.data(), sizeof(float) * std::min<size_t>(lut.size(), (size_t)std::max(cap, 0)));
    return (int)lut.size();
}

/* ComputeBatchRoad(): as ish_compute_batch with d_road [n] records / d_status [n] bytes on the device; road_out
 * [n][4] floats (vhor_image, tilt, height, alpha), status_out [n], alpha_ground [n]: from the copy the call fetched */
int ish_compute_batch_road(void* h, int pairwise, int n_images, const float* d_big, const int32_t* d_seg,
                           const void* d_road, const uint8_t* d_status, Section* sections, int* vhor_lib,
                           float* alpha_ground, float* road_out, uint8_t* status_out, int* triples, int cap,
                           int* counts, void* stream) {
    return guard([&] {
        Stixels* s = (Stixels*)h;
        std::vector<StixelsData> out;
        std::vector<Stixels::InstanceMapping> maps;
        std::vector<Stixels::RoadParameters> rp;
        std::vector<uint8_t> st;
        s->ComputeBatchRoad(pairwise != 0, n_images, d_big, d_seg, (const Stixels::RoadParameters*)d_road, d_status,
                            out, stream, triples ? &maps : nullptr, &rp, &st);
        for (int i = 0; i < n_images; i++) {
            std::memcpy(sections + (size_t)i * out[i].sections.size(), out[i].sections.data(),
                        out[i].sections.size() * sizeof(Section));
            vhor_lib[i] = out[i].vhor;
            alpha_ground[i] = out[i].alpha_ground;
            road_out[4 * i] = (float)rp[i].vhor; road_out[4 * i + 1] = rp[i].camera_tilt;
            road_out[4 * i + 2] = rp[i].camera_height; road_out[4 * i + 3] = rp[i].alpha_ground;
            status_out[i] = st[i];
            if (triples) {
                int n = 0;
                for (const auto& kv : maps[i]) {
                    if (n >= cap) break;
                    int* t = triples + ((size_t)i * cap + n) * 3;
                    t[0] = kv.first.first; t[1] = kv.first.second; t[2] = kv.second;
                    n++;
                }
                counts[i] = (int)maps[i].size();
            }
        }
    });
}

/* RoadEstimation::ComputeBatchDevice: d_road [n] records, d_status [n] bytes (device); fallback4 = (vhor_image, tilt,
 * height, alpha) */
int ire_compute_batch_device(void* h, const float* d_disparity, int n, void* d_road, uint8_t* d_status,
                             const float* fallback4, void* stream) {
    return guard([&] {
        const Stixels::RoadParameters fb = road_record(fallback4);
        ((RoadEstimation*)h)->ComputeBatchDevice(d_disparity, n, (Stixels::RoadParameters*)d_road, d_status, fb,
                                                 stream);
    });
}
/* RoadEstimation::ChooseLineShared with the pitch gate of Initialize(): returns the status (IS_ROAD_*); out: one
 * record; *index: the accepted line or -1 */
int ire_choose_line_shared(float cy, float baseline, float focal, int rows, const float* lines, int total,
                           int overflow, int max_lines, const float* fallback4, void* out, int* index) {
    float lo, hi;
    RoadEstimation::PitchGate(lo, hi);
    const Stixels::RoadParameters fb = road_record(fallback4);
    return RoadEstimation::ChooseLineShared(cy, baseline, focal, rows, lo, hi, lines, total, overflow, max_lines, fb,
                                            *(Stixels::RoadParameters*)out, index);
}
void ire_pitch_gate(float* lo, float* hi) { RoadEstimation::PitchGate(*lo, *hi); }

/* Times the road estimation + stixel computation of one resident batch, n_iter times, as a C++ caller's loop would
 * run it (outputs reused).  device_chain 0: RoadEstimation::ComputeBatch + Stixels::ComputeBatch; 1:
 * ComputeBatchDevice + ComputeBatchRoad on one stream (d_road [n] records, d_status [n] bytes: device scratch of the
 * caller).  One warm-up call, then s_each [n_iter]: seconds of every call by the host clock (each ends in the
 * synchronisation that delivers the Sections). */
int ish_time_road_chain(void* h, void* hre, int device_chain, int pairwise, int n_images, const float* d_big,
                        const int32_t* d_seg, void* d_road, uint8_t* d_status, const float* fallback4, int n_iter,
                        int with_instances, double* s_each) {
    return guard([&] {
        Stixels* s = (Stixels*)h;
        RoadEstimation* r = (RoadEstimation*)hre;
        const Stixels::RoadParameters fb = road_record(fallback4);
        std::vector<Stixels::RoadParameters> rp(n_images);
        std::vector<uint8_t> ok(n_images);
        std::vector<StixelsData> out;
        std::vector<Stixels::InstanceMapping> maps;
        /* one queue for both objects of the device chain: the order of the launches is all that joins them */
        void* chain = nullptr;
        if (device_chain && is_stream_create(&chain, 1) != IS_OK) throw std::runtime_error(is_last_error());
        struct Release { void* s; ~Release() { if (s) (void)is_stream_destroy(s); } } release{chain};
        for (int i = -1; i < n_iter; i++) {
            timespec t0, t1;
            clock_gettime(CLOCK_MONOTONIC, &t0);
            if (device_chain) {
                r->ComputeBatchDevice(d_big, n_images, (Stixels::RoadParameters*)d_road, d_status, fb, chain);
                s->ComputeBatchRoad(pairwise != 0, n_images, d_big, d_seg, (const Stixels::RoadParameters*)d_road,
                                    d_status, out, chain, with_instances ? &maps : nullptr);
            } else {
                r->ComputeBatch(d_big, n_images, rp.data(), ok.data(), nullptr);
                for (int k = 0; k < n_images; k++)
                    if (!ok[k]) rp[k] = fb; /* (what a live caller does with a frame without a road) */
                s->ComputeBatch(pairwise != 0, n_images, d_big, d_seg, rp.data(), out, nullptr,
                                with_instances ? &maps : nullptr);
            }
            clock_gettime(CLOCK_MONOTONIC, &t1);
            if (i >= 0) s_each[i] = (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec);
        }
    });
}

} /* extern "C" */
