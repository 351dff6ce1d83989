"""Ground-truth instance assignment of a batch on the device (f8, Stixels::AssignInstancesGTBatch; GPU box).

Prints one JSON line per mode (unary and pairwise preset): ms per batch of n frames for
- AssignInstancesGTBatch with its mapping (vote, pack, one copy, one synchronisation) and without (the vote alone,
  synchronised): host clock around the synchronised call, median of --iters after a warm-up, with the spread;
- yardstick (a): the numpy restatement tests/assign_gt_reference.py on the host, per batch (timed on the distinct
  frames, --host-repeats times, scaled to n), with its spread;
- the bytes of ground truth the vote touches (the clipped rectangles of the instance-class stixels) against the
  whole image, and the GB/s the vote alone achieves over the touched bytes;
- InstanceOverlapBatch on the same ground truth, so that a `rocprofv3 --kernel-trace --stats` run of this script
  shows k_iov (yardstick (b): it reads the image completely) beside k_assign_gt.
The device labels are checked against the restatement first.

    python tools/assign_gt_timing.py [--rows 1024 --cols 2048 --max-dis 128 --n 64 --iters 20]
"""
import argparse
import json
import os
import sys
import time

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
    import assign_gt_reference as ag
    import helpers
    import instance_eval_reference as ir
    import render_reference as rr
    from instance_stixels_amd import host, synthetic
    if not torch.cuda.is_available():
        sys.exit("assign_gt_timing.py needs a GPU")
    rows, cols, D, n = a.rows, a.cols, a.max_dis, a.n
    k = min(n, a.distinct)
    dev = torch.device("cuda", 0)
    for preset in ("drn_d_22_unary", "drn_d_38_pairwise"):
        case = helpers.build_case(preset, rows, cols, D, seed=1, n_images=1,
                                  size_filter=10 if preset.endswith("unary") else 8)
        cfg = case["cfg"]
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
        gt = torch.from_numpy(np.stack([gt_k[i % k] for i in range(n)])).to(dev)
        torch.cuda.synchronize()

        host_ms = []
        for _ in range(a.host_repeats):
            t0 = time.perf_counter()
            want = ag.assign(secs[:k], gt_k)
            host_ms.append((time.perf_counter() - t0) * 1e3 * n / k)
        got = st.AssignInstancesGTBatch(n, gt.data_ptr())
        same = got[:k] == ag.mappings(want[0]) and all(got[i] == got[i % k] for i in range(n))

        def timed(fn):
            for _ in range(3):
                fn()
            ts = []
            for _ in range(a.iters):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            return ts

        def vote_only():
            st.AssignInstancesGTBatch(n, gt.data_ptr(), with_mapping=False)
            torch.cuda.synchronize()

        with_map = timed(lambda: st.AssignInstancesGTBatch(n, gt.data_ptr()))
        alone = timed(vote_only)
        st.InstanceOverlapBatch(n, gt.data_ptr())   # k_iov on the same ground truth, for the kernel trace
        st.close()

        # the ground truth the vote touches: the clipped rectangles of the instance-class stixels
        w = cols // secs.shape[1]
        live = np.cumsum(secs["type"] == -1, axis=2) == 0
        inst = live & (secs["semantic_class"] >= 11) & (secs["semantic_class"] <= 18)
        height = np.clip(np.minimum(rows - 1 - secs["vB"].astype(np.int64), rows - 1)
                         - np.maximum(rows - 1 - secs["vT"].astype(np.int64), 0) + 1, 0, None)
        touched = int((height * inst).sum()) * w * 4
        med, med_alone = float(np.median(with_map)), float(np.median(alone))
        out = {"preset": preset, "shape": [rows, cols, D], "n": n, "iters": a.iters, "identical": bool(same),
               "stixels": int(live.sum()), "instance_class_stixels": int(inst.sum()),
               "labelled": int(sum(len(m) for m in got)),
               "assign_with_mapping_ms": round(med, 3), "assign_with_mapping_min_max": [round(min(with_map), 3),
                                                                                       round(max(with_map), 3)],
               "vote_alone_ms": round(med_alone, 3), "vote_alone_min_max": [round(min(alone), 3), round(max(alone), 3)],
               "host_restatement_ms_per_batch": round(float(np.median(host_ms)), 1),
               "host_restatement_min_max": [round(min(host_ms), 1), round(max(host_ms), 1)],
               "yardstick_a_met": bool(max(with_map) < min(host_ms)),
               "gt_bytes_touched": touched, "gt_bytes_image": 4 * n * rows * cols,
               "vote_alone_GBps_touched": round(touched / med_alone / 1e6, 1)}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
