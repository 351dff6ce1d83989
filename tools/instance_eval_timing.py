"""Instance overlap tables of a batch on the device (f6, Stixels::InstanceOverlapBatch; GPU box).

Prints one JSON line: ms per batch of n frames for InstanceOverlapBatch (tables of all frames, packed and copied
to the host: host clock around the synchronised call, median of --iters after a warm-up), the achieved GB/s of
the gt it reads (4 B per pixel), the records per frame, and the host side for contrast: the table-based AP of
evaluation.CityscapesInstanceEval per batch, and the numpy joint histogram per frame.  The gt is Cityscapes-like
(tests/instance_eval_reference.synth_gt: tens of instances, split / merged ones, groups, void, caravans).  The
device tables are checked against the numpy histogram on the first frames first.  Kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python tools/instance_eval_timing.py`.

    python tools/instance_eval_timing.py [--rows 1024 --cols 2048 --max-dis 128 --n 64 --iters 20]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

HBM_GBS = 6300.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--cols", type=int, default=2048)
    ap.add_argument("--max-dis", type=int, default=128)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    import torch
    import helpers
    import instance_eval_reference as ir
    import render_reference as rr
    from instance_stixels_amd import evaluation, host, synthetic
    if not torch.cuda.is_available():
        sys.exit("instance_eval_timing.py needs a GPU")
    rows, cols, D, n = a.rows, a.cols, a.max_dis, a.n
    case = helpers.build_case("drn_d_22_unary", rows, cols, D, seed=1, n_images=min(n, 4), size_filter=10)
    k = len(case["frames"])
    frames = [synthetic.make_frame(case["cfg"], seed=7 + i, n_slabs=12, offset_scale=1.0) for i in range(k)]
    dev = torch.device("cuda", 0)
    big = torch.from_numpy(np.stack([frames[i % k].disparity for i in range(n)])).to(dev)
    seg = torch.from_numpy(np.stack([frames[i % k].segmentation for i in range(n)])).to(dev)
    road = [(f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground) for f in (frames[i % k] for i in range(n))]
    st = host.Stixels()
    st.SetConfig(case["cfg"])
    st.Initialize(max_batch=n)
    data, maps = st.ComputeBatch(case["cfg"].pairwise, big.data_ptr(), seg.data_ptr(), road, with_instances=True)
    secs = np.stack([d.sections for d in data])
    inst = rr.render(secs[:k], rows, cols, maps[:k])[2]
    gt_k = ir.synth_gt(inst, seed=3)
    gt = torch.from_numpy(np.stack([gt_k[i % k] for i in range(n)])).to(dev)
    torch.cuda.synchronize()

    def tables():
        return st.InstanceOverlapBatch(n, gt.data_ptr())

    got = tables()
    t0 = time.perf_counter()
    want = [ir.joint_histogram(i, g) for i, g in zip(inst, gt_k)]
    numpy_ms = (time.perf_counter() - t0) * 1e3 / k
    same = all(np.array_equal(got[i], want[i]) for i in range(k))
    for _ in range(3):
        tables()
    ts = []
    for _ in range(a.iters):
        t0 = time.perf_counter()
        tables()
        ts.append((time.perf_counter() - t0) * 1e3)
    st.close()
    t0 = time.perf_counter()
    ev = evaluation.CityscapesInstanceEval()
    ev.add(got)
    res = ev.result()
    ap_ms = (time.perf_counter() - t0) * 1e3
    med = float(np.median(ts))
    px = n * rows * cols
    out = {"shape": [rows, cols, D], "n": n, "iters": a.iters, "identical_first_frames": bool(same),
           "tables_ms_per_batch": round(med, 3), "tables_ms_min": round(min(ts), 3),
           "gt_GBps": round(4 * px / med / 1e6, 1), "pct_of_hbm": round(100 * 4 * px / med / 1e6 / HBM_GBS, 1),
           "records_per_frame": int(np.median([len(t) for t in got])),
           "target_ms": 0.5, "target_met": bool(med <= 0.5),
           "host_ap_ms_per_batch": round(ap_ms, 1), "AP": res["AP"], "AP50": res["AP50"],
           "host_numpy_histogram_ms_per_frame": round(numpy_ms, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
