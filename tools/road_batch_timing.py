"""Road estimation of a batch of frames, per-frame path against the batched one (GPU box).

Prints one JSON line: ms per batch for RoadEstimation::Compute(device pointer) frame by frame and for
RoadEstimation::ComputeBatch, both on the same device-resident synthetic frames, after a warm-up, host clock
around calls that end in a synchronisation.  The outputs of the two paths are compared first.

    python tools/road_batch_timing.py [--rows 1024 --cols 2048 --max-dis 128 --n 64 --iters 10]
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
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    import numpy as np
    import torch
    import helpers
    from instance_stixels_amd import host
    if not torch.cuda.is_available():
        sys.exit("road_batch_timing.py needs a GPU")
    rows, cols, D, n = a.rows, a.cols, a.max_dis, a.n
    case = helpers.build_case("drn_d_22_unary", rows, cols, D, seed=1, n_images=min(n, 8))
    disp = np.stack([case["disparity"][i % len(case["frames"])] for i in range(n)])
    cfg = case["cfg"]
    d = torch.from_numpy(disp).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    re_ = host.RoadEstimation()
    re_.Initialize(cfg.camera_center_y * rows / 1024, cfg.baseline, cfg.focal, rows, cols, D)
    step = rows * cols * 4

    def per_frame():
        return [(re_.ComputeOnDevice(d.data_ptr() + i * step),
                 (re_.horizon_point, re_.pitch, re_.camera_height, re_.slope)) for i in range(n)]

    def batched():
        return re_.ComputeBatch(d.data_ptr(), n)

    single = per_frame()
    road, ok = batched()
    same = all(ok[i] == s[0] and (not s[0] or road[i] == s[1]) for i, s in enumerate(single))
    res = {}
    for name, fn in (("per_frame", per_frame), ("batched", batched)):
        fn()
        ts = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        res[name] = ts
    fallbacks = re_.GetBatchFallbacks()
    re_.close()
    med = {k: float(np.median(v)) for k, v in res.items()}
    print(json.dumps({
        "shape": [rows, cols, D], "n": n, "iters": a.iters, "identical": bool(same),
        "frames_ok": int(sum(ok)), "batch_fallbacks": fallbacks,
        "per_frame_ms_per_batch": round(med["per_frame"], 3), "batched_ms_per_batch": round(med["batched"], 3),
        "per_frame_ms_min": round(min(res["per_frame"]), 3), "batched_ms_min": round(min(res["batched"]), 3),
        "speedup": round(med["per_frame"] / med["batched"], 1)}))


if __name__ == "__main__":
    main()
