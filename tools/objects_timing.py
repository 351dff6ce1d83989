"""The per-instance objects and contours of a batch from the device (Stixels::InstanceObjectsBatch) against the two
ways to the same data that existed before it (GPU box).

Prints one JSON line per preset and instance map (the cluster labels; the ground-truth vote of
AssignInstancesGTBatch over instance_eval_reference.synth_gt), at 1024x2048x128 and 64 frames (4 distinct) by
default.  Every figure is the host clock around a call that ends in a synchronisation, after a warm-up; median
[min, max] over --iters rounds, all forms in turn in the same rounds:
  objects_ms       Python host.Stixels.InstanceObjectsBatch(n): the device reduction, ONE copy of the block to pinned
                   memory, one synchronisation, and the copies into fresh numpy arrays
  objects_view_ms  ish_instance_objects_batch alone (C++ Stixels::InstanceObjectsBatchView): the records left in the
                   object's pinned buffer
  (a) world_view_ms     ish_world_batch alone (C++ Stixels::WorldBatchView): the floor of anything that starts from
                        the per-stixel records
  (b) world_reduce_ms   host.Stixels.WorldBatch(n, out=array kept between the rounds) plus a vectorised numpy
                        reduction of its records to the same objects and points (reduce_ms: the reduction alone)
`below_world_view` = (a) median - objects_ms median exceeds the larger of the two spreads (max - min), the rule of
DESIGN.md section 10d.  The objects are verified first: bytewise against tests/objects_reference.py on the first
--verify frames, and field by field against the numpy reduction of (b) on all frames.
For kernel times run `rocprofv3 --kernel-trace --stats -- python tools/objects_timing.py --device-only`
(k_obj_columns, k_obj_count, k_obj_emit and the memset of the key table).

    python tools/objects_timing.py [--rows 1024 --cols 2048 --max-dis 128 --n 64 --iters 20]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def stat(ts):
    import numpy as np
    return [round(float(np.median(ts)), 3), round(float(np.min(ts)), 3), round(float(np.max(ts)), 3)]


def reduce_world(offsets, records, rows, width):
    """The per-stixel records of WorldBatch reduced to objects and points on the host, vectorised: what a consumer
    of per-instance results had to do.  Returns (key [m] = frame*8000 + (class-11)*1000 + label ascending, n_stixels,
    pixels, col_min, col_max, top, bottom, q16, point key [p] = key*2^20 + column ascending, point section)."""
    import numpy as np
    frame = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    cls, label = records["semantic_class"], records["instance_id"]
    member = (cls >= 11) & (cls <= 18) & (label >= 0) & (label < 1000)
    r, frame = records[member], frame[member]
    key = frame.astype(np.int64) * 8000 + (r["semantic_class"].astype(np.int64) - 11) * 1000 + r["instance_id"]
    top = np.maximum(rows - 1 - r["vT"].astype(np.int64), 0)
    bot = np.minimum(rows - 1 - r["vB"].astype(np.int64), rows - 1)
    height = np.maximum(bot - top + 1, 0)
    d = r["disparity"]
    with np.errstate(invalid="ignore"):
        q = np.where((d >= 0) & (d < 32768), np.rint(d.astype(np.float64) * 65536.0), 0).astype(np.int64) * height
    keys, inverse, counts = np.unique(key, return_inverse=True, return_counts=True)
    m = len(keys)
    pixels = np.bincount(inverse, height * width, m).astype(np.int64)
    q16 = np.zeros(m, np.int64)
    np.add.at(q16, inverse, q)
    col_min, col_max = np.full(m, 1 << 30), np.full(m, -1)
    np.minimum.at(col_min, inverse, r["column"])
    np.maximum.at(col_max, inverse, r["column"])
    t, b = np.full(m, rows), np.full(m, -1)
    some = height > 0
    np.minimum.at(t, inverse[some], top[some])
    np.maximum.at(b, inverse[some], bot[some])
    # per (key, column) the member with the largest disparity, the smaller section on a tie
    pkey = key * (1 << 20) + r["column"]
    order = np.lexsort((r["section"], -d.astype(np.float64), pkey))
    first = np.ones(len(order), bool)
    first[1:] = pkey[order][1:] != pkey[order][:-1]
    return keys, counts, pixels, col_min, col_max, t, b, q16, pkey[order][first], r["section"][order][first]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--cols", type=int, default=2048)
    ap.add_argument("--max-dis", type=int, default=128)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--verify", type=int, default=2, help="frames compared bytewise with tests/objects_reference.py")
    ap.add_argument("--presets", default="drn_d_22_unary,drn_d_38_pairwise")
    ap.add_argument("--maps", default="cluster,gt", help="instance ids: the cluster labels, the ground-truth vote")
    ap.add_argument("--device-only", action="store_true", help="only InstanceObjectsBatch (for a profiler run)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import helpers
    import instance_eval_reference as ir
    import objects_reference as orf
    import render_reference as rr
    from instance_stixels_amd import host, synthetic
    if not torch.cuda.is_available():
        sys.exit("objects_timing.py needs a GPU")
    rows, cols, D, n = a.rows, a.cols, a.max_dis, a.n
    dev = torch.device("cuda", 0)
    L = host.lib()
    for preset, mode in [(p, m) for p in a.presets.split(",") for m in a.maps.split(",")]:
        k = min(n, 4)
        case = helpers.build_case(preset, rows, cols, D, seed=1, n_images=1,
                                  size_filter=10 if preset.endswith("unary") else 8)
        cfg = case["cfg"]
        # frames with instance offsets, so that clusters form (as tools/assign_gt_timing.py)
        frames = [synthetic.make_frame(cfg, seed=7 + i, n_slabs=12, offset_scale=1.0) for i in range(k)]
        big = torch.from_numpy(np.stack([frames[i % k].disparity for i in range(n)])).to(dev)
        seg = torch.from_numpy(np.stack([frames[i % k].segmentation for i in range(n)])).to(dev)
        road = [(f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground)
                for f in (frames[i % k] for i in range(n))]
        st = host.Stixels()
        st.SetConfig(cfg)
        st.Initialize(max_batch=n)
        data, maps = st.ComputeBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), road, with_instances=True)
        if mode == "gt":  # the ground-truth vote over a Cityscapes-like gt drawn from the clusters
            secs_k = np.stack([d.sections for d in data[:k]])
            gt_k = ir.synth_gt(rr.render(secs_k, rows, cols, maps[:k])[2], seed=3)
            gt = torch.from_numpy(np.stack([gt_k[i % k] for i in range(n)])).to(dev)
            torch.cuda.synchronize()
            maps = st.AssignInstancesGTBatch(n, gt.data_ptr())
        width = cols // st.GetRealCols()
        objects, points, frame_objects, frame_points = st.InstanceObjectsBatch(n)
        v = min(a.verify, n)
        secs = np.stack([d.sections for d in data[:v]])
        want = orf.objects_and_points(secs, orf.mapping_to_map(maps[:v], secs.shape), rows, cols)
        assert len(want[0]) > 0, "the first frames hold no object: nothing is verified"
        assert objects[:len(want[0])].tobytes() == want[0].tobytes(), "objects differ from the restatement"
        assert points[:len(want[1])].tobytes() == want[1].tobytes(), "points differ from the restatement"
        out = {"preset": preset, "map": mode, "shape": [rows, cols, D], "n": n, "iters": a.iters,
               "objects": len(objects), "points": len(points), "member_stixels": int(objects["n_stixels"].sum()),
               "objects_per_frame": round(len(objects) / n, 1), "points_per_frame": round(len(points) / n, 1),
               "object_bytes": len(objects) * 64 + len(points) * 32, "frames_verified_bytewise": v}
        if a.device_only:
            for _ in range(a.iters):
                st.InstanceObjectsBatch(n)
            st.close()
            print(json.dumps(out), flush=True)
            continue
        offsets, records = st.WorldBatch(n)
        keep = np.empty(len(records), host.WORLD_DTYPE)
        out.update(world_records=len(records), world_bytes=len(records) * 96)
        # the numpy reduction of the world records gives the device's objects
        keys, counts, pixels, cmin, cmax, top, bot, q16, pkey, psec = reduce_world(offsets, records, rows, width)
        okey = (objects["frame"].astype(np.int64) * 8000 + (objects["semantic_class"].astype(np.int64) - 11) * 1000
                + objects["label"])
        same = (np.array_equal(keys, okey) and np.array_equal(counts, objects["n_stixels"])
                and np.array_equal(pixels, objects["pixels"]) and np.array_equal(cmin, objects["col_min"])
                and np.array_equal(cmax, objects["col_max"]) and np.array_equal(top, objects["top"])
                and np.array_equal(bot, objects["bottom"]) and np.array_equal(q16, objects["disparity_q16_sum"])
                and np.array_equal(pkey, okey[points["object"]] * (1 << 20) + points["column"])
                and np.array_equal(psec, points["section"]))
        out["reduction_identical"] = bool(same)
        fo, fp, totals = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(2, np.int32)
        woff = np.zeros(n + 1, np.int32)
        t = {key: [] for key in ("objects_ms", "objects_view_ms", "world_view_ms", "world_reduce_ms", "reduce_ms")}
        for it in range(-3, a.iters):
            t0 = time.perf_counter()
            st.InstanceObjectsBatch(n)
            t1 = time.perf_counter()
            rc1 = L.ish_instance_objects_batch(st._h, n, fo.ctypes.data, fp.ctypes.data, totals.ctypes.data, None)
            t2 = time.perf_counter()
            rc2 = L.ish_world_batch(st._h, n, woff.ctypes.data, None)
            t3 = time.perf_counter()
            o, r = st.WorldBatch(n, out=keep)
            t4 = time.perf_counter()
            reduce_world(o, r, rows, width)
            t5 = time.perf_counter()
            assert rc1 == 0 and rc2 == 0
            if it >= 0:
                for key, ms in zip(t, (t1 - t0, t2 - t1, t3 - t2, t5 - t3, t5 - t4)):
                    t[key].append(ms * 1e3)
        for key, ts in t.items():
            out[key] = stat(ts)
        spread = max(max(t["objects_ms"]) - min(t["objects_ms"]), max(t["world_view_ms"]) - min(t["world_view_ms"]))
        out["below_world_view"] = bool(np.median(t["world_view_ms"]) - np.median(t["objects_ms"]) > spread)
        st.close()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
