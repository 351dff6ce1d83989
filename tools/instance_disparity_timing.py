"""Clustering in (x, y, instance disparity) of a batch on the device (f10, Stixels::ClusterInstanceDisparityBatch;
GPU box).

Prints one JSON line per mode (unary and pairwise preset): ms per batch of n frames for
- ClusterInstanceDisparityBatch on resident images without its mapping (six kinds of launch, the copy of the key
  counts, one synchronisation), with its mapping, and on host arrays (the two copies included): host clock around the
  synchronised call, median of --iters after a warm-up, with the spread;
- yardstick (a): the numpy restatement tests/instance_disparity_reference.py on the host, per batch (timed on the
  distinct frames, --host-repeats times, scaled to n; numpy's own threads, 16 at most), with its spread;
- yardstick (b): ReclusterBatch on the same batch with the same three parameters, synchronised: what the two median
  stages add over the clustering alone;
- yardstick (c): the bytes of ground truth the stixel walk touches (the clipped rectangles of the instance-class
  stixels: those k_assign_gt touches) -- AssignInstancesGTBatch runs once on the same ground truth, so that a
  `rocprofv3 --kernel-trace --stats` run of this script shows k_assign_gt beside k_idisp_stixel and the bytes per
  second of both follow from the trace.
The device labels and medians are checked against the restatement first.

    python tools/instance_disparity_timing.py [--rows 1024 --cols 2048 --max-dis 128 --n 64 --iters 20]
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--cols", type=int, default=2048)
    ap.add_argument("--max-dis", type=int, default=128)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    import helpers
    import instance_disparity_reference as idr
    import instance_eval_reference as ir
    import render_reference as rr
    from instance_stixels_amd import host, synthetic
    if not torch.cuda.is_available():
        sys.exit("instance_disparity_timing.py needs a GPU")
    rows, cols, D, n = a.rows, a.cols, a.max_dis, a.n
    k = min(n, a.distinct)
    dev = torch.device("cuda", 0)
    for preset in ("drn_d_22_unary", "drn_d_38_pairwise"):
        case = helpers.build_case(preset, rows, cols, D, seed=1, n_images=1,
                                  size_filter=10 if preset.endswith("unary") else 8)
        cfg = case["cfg"]
        par = dict(eps=float(cfg.eps), min_pts=int(cfg.min_pts), size_filter=int(cfg.size_filter))
        frames = [synthetic.make_frame(cfg, seed=7 + i, n_slabs=12, offset_scale=1.0) for i in range(k)]
        big = torch.from_numpy(np.stack([frames[i % k].disparity for i in range(n)])).to(dev)
        seg = torch.from_numpy(np.stack([frames[i % k].segmentation for i in range(n)])).to(dev)
        road = [(f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground)
                for f in (frames[i % k] for i in range(n))]
        st = host.Stixels()
        st.SetConfig(cfg)
        st.Initialize(max_batch=n)
        data, maps = st.ComputeBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), road, with_instances=True)
        secs = np.stack([d.sections for d in data])
        gt_k = ir.synth_gt(rr.render(secs[:k], rows, cols, maps[:k])[2], seed=3)
        disp_k = np.clip(np.rint(np.nan_to_num(np.stack([f.disparity for f in frames]))), 0, 255).astype(np.uint8)
        disp_k[np.random.default_rng(5).random(disp_k.shape) < 0.04] = 0
        gt_h = np.stack([gt_k[i % k] for i in range(n)])
        disp_h = np.stack([disp_k[i % k] for i in range(n)])
        gt, disp = torch.from_numpy(gt_h).to(dev), torch.from_numpy(disp_h).to(dev)
        torch.cuda.synchronize()

        host_ms = []
        for _ in range(a.host_repeats):
            t0 = time.perf_counter()
            want = idr.run(secs[:k], gt_k, disp_k, **par)
            host_ms.append((time.perf_counter() - t0) * 1e3 * n / k)
        got, med = st.ClusterInstanceDisparityBatch(n, gt.data_ptr(), disp.data_ptr(), **par, with_stixel_median=True)
        same = (got[:k] == want["mappings"] and all(got[i] == got[i % k] for i in range(n)) and
                np.array_equal(med[:k].view(np.uint32), want["stixel_median"].view(np.uint32)))

        def timed(fn):
            for _ in range(3):
                fn()
            ts = []
            for _ in range(a.iters):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            return ts

        def recluster():
            st.ReclusterBatch(with_mapping=False, **par)
            torch.cuda.synchronize()

        alone = timed(lambda: st.ClusterInstanceDisparityBatch(n, gt.data_ptr(), disp.data_ptr(), **par,
                                                               with_mapping=False))
        with_map = timed(lambda: st.ClusterInstanceDisparityBatch(n, gt.data_ptr(), disp.data_ptr(), **par))
        from_host = timed(lambda: st.ClusterInstanceDisparityBatch(n, gt_h, disp_h, **par, with_mapping=False))
        recl = timed(recluster)
        st.AssignInstancesGTBatch(n, gt.data_ptr(), with_mapping=False)   # k_assign_gt, for the kernel trace
        torch.cuda.synchronize()
        st.close()

        w = cols // secs.shape[1]
        live = np.cumsum(secs["type"] == -1, axis=2) == 0
        inst = live & (secs["semantic_class"] >= 11) & (secs["semantic_class"] <= 18)
        height = np.clip(np.minimum(rows - 1 - secs["vB"].astype(np.int64), rows - 1)
                         - np.maximum(rows - 1 - secs["vT"].astype(np.int64), 0) + 1, 0, None)
        touched = int((height * inst).sum()) * w * 4

        def mmm(ts, digits=3):
            return [round(float(np.median(ts)), digits), round(min(ts), digits), round(max(ts), digits)]

        out = {"preset": preset, "shape": [rows, cols, D], "n": n, "iters": a.iters, "identical": bool(same),
               "instance_class_stixels": int(inst.sum()), "keys_per_frame_max": int(want["key_count"].max()),
               "labelled": int(sum(sum(v >= 0 for v in m.values()) for m in got)),
               "cluster_disparity_ms_med_min_max": mmm(alone), "with_mapping_ms_med_min_max": mmm(with_map),
               "from_host_arrays_ms_med_min_max": mmm(from_host), "recluster_ms_med_min_max": mmm(recl),
               "host_restatement_ms_per_batch_med_min_max": mmm(host_ms, 1),
               "yardstick_a_device_with_copies_below_host": bool(max(from_host) < min(host_ms)),
               "gt_bytes_touched_by_the_stixel_walk": touched, "gt_bytes_image": 4 * n * rows * cols,
               "pixel_pass_bytes": 2 * 4 * n * rows * cols + n * rows * cols}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
