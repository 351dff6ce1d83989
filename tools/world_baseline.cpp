/* world_baseline.cpp -- the C++ half of tools/world_timing.py (built by it with g++ against libInstanceStixels.so;
 * no part of the shipped libraries).  One ComputeBatch with instances, then n_iter rounds (after two warm-up rounds)
 * that time, in turn, with the host clock:
 *   view_ms    Stixels::WorldBatchView(n): launches, the copy to pinned memory, the synchronisation
 *   reuse_ms   Stixels::WorldBatch(n, world): the same plus one copy into a World that keeps its capacity
 *   value_ms   Stixels::WorldBatch(n) by value, the result released inside the timed region
 *   host_ms    THE BASELINE, the host composition that existed before: per frame Get3DVertices(out[i]) plus one
 *              instance_stixels[i] lookup per stixel into a vector of is_world_stixel per frame, the frames over
 *              `threads` host threads; the per-frame vectors keep their capacity from round to round, as the World
 *              of reuse_ms does; the clock stops when the threads have joined
 *   concat_ms  on top of host_ms: the frames' vectors copied back to back into one array (what a consumer that
 *              wants the batch as ONE array, like WorldBatch's result, would add; the ROS node does not)
 * identical: 1 when the device records and the host composition of the last round are the same bytes outside NaN
 * vertices. */
#include <cstddef>
#include <cstring>
#include <ctime>
#include <exception>
#include <thread>
#include <vector>

#include "instance_stixels_core.h"
#include "InstanceStixels/Stixels.hpp"

static double now_ms() {
    timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}

extern "C" int wt_time_world(void* h, int pairwise, int n_images, const float* d_big, const int32_t* d_seg,
                             const float* road, int n_iter, int threads, double* view_ms, double* reuse_ms,
                             double* value_ms, double* host_ms, double* concat_ms, int64_t* n_records,
                             int* identical) {
    try {
        Stixels* s = (Stixels*)h;
        std::vector<Stixels::RoadParameters> rp(n_images);
        for (int i = 0; i < n_images; i++)
            rp[i] = Stixels::RoadParameters{(int)road[4 * i], road[4 * i + 1], road[4 * i + 2], road[4 * i + 3]};
        std::vector<StixelsData> out;
        std::vector<Stixels::InstanceMapping> maps;
        s->ComputeBatch(pairwise != 0, n_images, d_big, d_seg, rp.data(), out, nullptr, &maps);
        const int C = s->GetRealCols(), S = s->GetMaxSections();
        auto compose_frame = [&](int f, std::vector<is_world_stixel>& rec) {
            const std::vector<float> v = s->Get3DVertices(out[f]);
            rec.clear();
            rec.reserve(v.size() / 12);
            const Stixels::InstanceMapping& m = maps[f];
            for (int c = 0; c < C; c++)
                for (int j = 0; j < S; j++) {
                    const Section& sec = out[f].sections[(size_t)c * S + j];
                    if (sec.type == -1) break;
                    is_world_stixel r;
                    r.column = c; r.section = j; r.type = sec.type; r.vB = sec.vB; r.vT = sec.vT;
                    r.semantic_class = sec.semantic_class;
                    const auto it = m.find(std::make_pair(c, j));
                    r.instance_id = it == m.end() ? -1 : it->second;
                    r.disparity = sec.disparity; r.cost = sec.cost;
                    r.instance_meanx = sec.instance_meanx; r.instance_meany = sec.instance_meany;
                    std::memcpy(r.vertices, v.data() + 12 * rec.size(), sizeof(r.vertices));
                    r.reserved = 0;
                    rec.push_back(r);
                }
        };
        if (threads < 1) threads = 1;
        Stixels::World w, hw;
        std::vector<int32_t> view_offsets;
        std::vector<std::vector<is_world_stixel>> frames(n_images); /* keep their capacity, like w */
        for (int it = -2; it < n_iter; it++) {
            const double t0 = now_ms();
            s->WorldBatchView(n_images, view_offsets);
            const double t1 = now_ms();
            s->WorldBatch(n_images, w);
            const double t2 = now_ms();
            { const Stixels::World fresh = s->WorldBatch(n_images); }
            const double t3 = now_ms();
            std::vector<std::thread> pool;
            for (int t = 0; t < threads; t++)
                pool.emplace_back([&, t] { for (int f = t; f < n_images; f += threads) compose_frame(f, frames[f]); });
            for (auto& t : pool) t.join();
            const double t4 = now_ms();
            hw.frame_offsets.assign(n_images + 1, 0);
            for (int f = 0; f < n_images; f++)
                hw.frame_offsets[f + 1] = hw.frame_offsets[f] + (int32_t)frames[f].size();
            hw.stixels.resize((size_t)hw.frame_offsets[n_images]);
            for (int f = 0; f < n_images; f++)
                if (!frames[f].empty())
                    std::memcpy(hw.stixels.data() + hw.frame_offsets[f], frames[f].data(),
                                frames[f].size() * sizeof(is_world_stixel));
            const double t5 = now_ms();
            if (it >= 0) {
                view_ms[it] = t1 - t0; reuse_ms[it] = t2 - t1; value_ms[it] = t3 - t2;
                host_ms[it] = t4 - t3; concat_ms[it] = t5 - t4;
            }
        }
        *n_records = (int64_t)w.stixels.size();
        bool same = w.frame_offsets == hw.frame_offsets && view_offsets == w.frame_offsets;
        for (size_t r = 0; same && r < w.stixels.size(); r++) {
            const is_world_stixel &x = w.stixels[r], &y = hw.stixels[r];
            same = std::memcmp(&x, &y, offsetof(is_world_stixel, vertices)) == 0 && x.reserved == y.reserved;
            for (int k = 0; same && k < 12; k++)
                same = (x.vertices[k] != x.vertices[k] && y.vertices[k] != y.vertices[k]) ||
                       std::memcmp(&x.vertices[k], &y.vertices[k], 4) == 0;
        }
        *identical = same ? 1 : 0;
        return 0;
    } catch (const std::exception&) {
        return -1;
    }
}
