"""Rendering and scoring a batch of stixel results on the device (f5, Stixels::RenderBatch; GPU box).

Prints one JSON line: ms per batch of n frames for RenderBatch writing the three images (label, disparity,
instance), for the metrics alone (confusion matrix + disparity deviation against ground truth), and for both
together, with the achieved GB/s of the bytes each moves (9 B per pixel written, 5 B per pixel of ground truth
read) against the 6.3 TB/s achievable HBM bandwidth; then the numpy restatement of tests/render_reference.py
on the host, per frame, for contrast.  Host clock around calls that end in a synchronisation, after a warm-up;
the Sections are those of one ComputeBatch of the same frames.  The device images are checked against the
restatement on the first frame first.

    python tools/render_timing.py [--rows 1024 --cols 2048 --max-dis 128 --n 64 --iters 20]
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
    ap.add_argument("--host-frames", type=int, default=2)
    a = ap.parse_args()
    import numpy as np
    import torch
    import helpers
    import render_reference as rr
    from instance_stixels_amd import host
    if not torch.cuda.is_available():
        sys.exit("render_timing.py needs a GPU")
    rows, cols, D, n = a.rows, a.cols, a.max_dis, a.n
    case = helpers.build_case("drn_d_22_unary", rows, cols, D, seed=1, n_images=min(n, 8), size_filter=10)
    k = len(case["frames"])
    dev = torch.device("cuda", 0)
    big = torch.from_numpy(np.stack([case["disparity"][i % k] for i in range(n)])).to(dev)
    seg = torch.from_numpy(np.stack([case["segmentation"][i % k] for i in range(n)])).to(dev)
    road = [(f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground)
            for f in (case["frames"][i % k] for i in range(n))]
    st = host.Stixels()
    st.SetConfig(case["cfg"])
    st.Initialize(max_batch=n)
    data, maps = st.ComputeBatch(case["cfg"].pairwise, big.data_ptr(), seg.data_ptr(), road, with_instances=True)
    secs = np.stack([d.sections for d in data])

    label = torch.empty((n, rows, cols), dtype=torch.uint8, device=dev)
    disp = torch.empty((n, rows, cols), dtype=torch.float32, device=dev)
    inst = torch.empty((n, rows, cols), dtype=torch.int32, device=dev)
    conf = torch.zeros((34, 34), dtype=torch.int64, device=dev)
    w0 = rr.render(secs[:1], rows, cols, maps[:1])
    rng = np.random.default_rng(0)
    gt1 = np.where(rng.random(w0[0].shape) < 0.1, 255, w0[0]).astype(np.uint8)
    gd1 = (w0[1] + rng.normal(0, 0.5, w0[1].shape)).astype(np.float32)
    gt = torch.from_numpy(gt1).to(dev).expand(n, rows, cols).contiguous()
    gd = torch.from_numpy(gd1).to(dev).expand(n, rows, cols).contiguous()
    torch.cuda.synchronize()

    def images():
        return st.RenderBatch(n, label=label.data_ptr(), disparity=disp.data_ptr(), instance=inst.data_ptr())

    def metrics():
        return st.RenderBatch(n, gt_label=gt.data_ptr(), confusion=conf.data_ptr(), gt_disparity=gd.data_ptr())

    def both():
        return st.RenderBatch(n, label=label.data_ptr(), disparity=disp.data_ptr(), instance=inst.data_ptr(),
                              gt_label=gt.data_ptr(), confusion=conf.data_ptr(), gt_disparity=gd.data_ptr())

    both()
    same = (np.array_equal(label[0].cpu().numpy(), w0[0][0]) and np.array_equal(inst[0].cpu().numpy(), w0[2][0])
            and np.array_equal(disp[0].cpu().numpy().view(np.int32), w0[1][0].view(np.int32)))
    px = n * rows * cols
    nbytes = {"images": 9 * px, "metrics": 5 * px, "both": 14 * px}
    res = {}
    for name, fn in (("images", images), ("metrics", metrics), ("both", both)):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        res[name] = ts
    st.close()
    med = {k: float(np.median(v)) for k, v in res.items()}

    t0 = time.perf_counter()
    hf = a.host_frames
    for i in range(hf):
        w = rr.render(secs[i:i + 1], rows, cols, maps[i:i + 1])
        rr.confusion(w[0], gt1, 34)
        rr.deviation(w[1], gd1)
    host_ms = (time.perf_counter() - t0) * 1e3 / hf

    out = {"shape": [rows, cols, D], "n": n, "iters": a.iters, "identical_frame0": bool(same)}
    for k in ("images", "metrics", "both"):
        out[f"{k}_ms_per_batch"] = round(med[k], 3)
        out[f"{k}_ms_min"] = round(min(res[k]), 3)
        out[f"{k}_GBps"] = round(nbytes[k] / med[k] / 1e6, 1)
        out[f"{k}_pct_of_hbm"] = round(100 * nbytes[k] / med[k] / 1e6 / HBM_GBS, 1)
    out["host_numpy_ms_per_frame"] = round(host_ms, 1)
    out["host_numpy_ms_per_batch_est"] = round(host_ms * n, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
