"""Ground-truth offset targets and CNN offset channels of a batch on the device (f11: is_mode_downsample,
is_gt_instance_targets, Stixels::GroundTruthOffsetsBatch; GPU box).

Prints one JSON line: ms per batch of n frames, host clock around the synchronised call, median of --iters after a
warm-up, with min and max, for
- core.gt_instance_targets on resident images: 2 planes + ids + segmentation channels; the same with the raw
  disparity (3 planes; the key counts are read back, one synchronisation more);
- Stixels::GroundTruthOffsetsBatch (the segmentation channels alone, the object's scratch);
- core.mode_downsample of the int32 ground truth alone, and the bytes per second that is (yardstick (b): the kernel
  reads what k_iov reads; the kernel's own time comes from a `rocprofv3 --kernel-trace --stats` run of this script);
- yardstick (a): the numpy restatement tests/gt_targets_reference.py on the host, per batch (timed on the distinct
  frames, --host-repeats times, scaled to n), with its spread.
The device outputs are checked against the restatement first.  The ground truth is instance_eval_reference.synth_gt of
the rendered instance image of a batch of synthetic frames; --save-gt writes the distinct frames to an .npz.

Without a GPU, --host-only --load-gt FILE times the restatement on those frames, and with --reference DIR (a checkout
of the reference) once its own three functions, cut out of its sources as
tests/golden/reference_python_targets/make_golden.py does.

    python tools/gt_targets_timing.py [--rows 1024 --cols 2048 --max-dis 128 --n 64 --iters 20]
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def mmm(ts, digits=3):
    import numpy as np
    return [round(float(np.median(ts)), digits), round(min(ts), digits), round(max(ts), digits)]


def host_yardstick(a, gt_k, disp_k, n):
    """The restatement (and once the reference's functions) on the distinct frames, scaled to n frames."""
    import numpy as np
    import gt_targets_reference as gr
    k = gt_k.shape[0]
    p2s = 1 << int(np.ceil(np.log2(gt_k.shape[1] // 8)))   # (any power of two > rows / 8 serves the host timing)
    out = {}
    for name, d in (("offsets", None), ("offsets_and_disparity", disp_k)):
        ms = []
        for _ in range(a.host_repeats):
            t0 = time.perf_counter()
            t, _ = gr.targets(gt_k, d)
            gr.as_prediction(np.zeros((k, gt_k.shape[2] // 8, 21, 2 * p2s), np.int32), t[:, -2:])
            ms.append((time.perf_counter() - t0) * 1e3 * n / k)
        out[f"host_restatement_{name}_ms_per_batch_med_min_max"] = mmm(ms, 1)
    if a.reference:
        sys.path.insert(0, os.path.join(ROOT, "tests", "golden", "reference_python_targets"))
        os.environ["REFERENCE"] = a.reference
        import torch
        import make_golden
        mode, off2, off3 = make_golden.reference_functions()
        t0 = time.perf_counter()
        ids8 = mode(None, gt_k[0], 8)
        t1 = time.perf_counter()
        o2 = off2(None, torch.from_numpy(ids8.copy())).numpy()
        t2 = time.perf_counter()
        d8 = mode(None, disp_k[0], 8)
        o3 = off3(None, torch.from_numpy(ids8.copy()), torch.from_numpy(d8.astype(np.float32))).numpy()
        t3 = time.perf_counter()
        want, _ = gr.targets(gt_k[:1], disp_k[:1])
        out["reference_python_one_frame_s"] = dict(modefilter_np=round(t1 - t0, 3), instance_offsets=round(t2 - t1, 3),
                                                   mode_and_offsets_disparity=round(t3 - t2, 3))
        out["reference_python_ms_per_batch"] = round((t2 - t0) * 1e3 * n, 1)
        out["reference_python_identical"] = bool(np.array_equal(o2.view(np.uint32), want[0, 1:].view(np.uint32)) and
                                                 np.array_equal(o3.view(np.uint32), want[0].view(np.uint32)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--cols", type=int, default=2048)
    ap.add_argument("--max-dis", type=int, default=128)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--save-gt")
    ap.add_argument("--load-gt")
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--reference")
    ap.add_argument("--no-host", action="store_true", help="skip yardstick (a): for runs under a profiler")
    a = ap.parse_args()
    import numpy as np
    if a.host_only:
        z = np.load(a.load_gt)
        gt_k, disp_k = z["gt"].astype(np.int32), z["disparity"]
        out = {"shape": list(gt_k.shape[1:]), "n": a.n, "distinct": int(gt_k.shape[0])}
        out.update(host_yardstick(a, gt_k, disp_k, a.n))
        print(json.dumps(out), flush=True)
        return
    import torch
    import gt_targets_reference as gr
    import helpers
    import instance_eval_reference as ir
    import render_reference as rr
    from instance_stixels_amd import core, host, synthetic
    if not torch.cuda.is_available():
        sys.exit("gt_targets_timing.py needs a GPU (or --host-only --load-gt FILE)")
    rows, cols, D, n = a.rows, a.cols, a.max_dis, a.n
    k = min(n, a.distinct)
    dev = torch.device("cuda", 0)
    case = helpers.build_case("drn_d_22_unary", rows, cols, D, seed=1, n_images=1, size_filter=10)
    cfg = case["cfg"]
    frames = [synthetic.make_frame(cfg, seed=7 + i, n_slabs=12, offset_scale=1.0) for i in range(k)]
    big = torch.from_numpy(np.stack([f.disparity for f in frames])).to(dev)
    seg_k = np.stack([f.segmentation for f in frames])
    road = [(f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground) for f in frames]
    st = host.Stixels()
    st.SetConfig(cfg)
    st.Initialize(max_batch=n)
    data, maps = st.ComputeBatch(cfg.pairwise, big.data_ptr(), torch.from_numpy(seg_k).to(dev).data_ptr(), road,
                                 with_instances=True)
    secs = np.stack([d.sections for d in data])
    gt_k = np.clip(ir.synth_gt(rr.render(secs, rows, cols, maps)[2], seed=3), 0, 65535).astype(np.int32)
    disp_k = (np.clip(np.nan_to_num(np.stack([f.disparity for f in frames])), 0, 255) * 256).astype(np.uint16)
    disp_k[np.random.default_rng(5).random(disp_k.shape) < 0.04] = 0
    if a.save_gt:
        np.savez_compressed(a.save_gt, gt=gt_k.astype(np.uint16), disparity=disp_k)
    gt = torch.from_numpy(np.stack([gt_k[i % k] for i in range(n)])).to(dev)
    disp = torch.from_numpy(np.stack([disp_k[i % k] for i in range(n)])).to(dev)
    seg = torch.from_numpy(np.stack([seg_k[i % k] for i in range(n)])).to(dev)
    torch.cuda.synchronize()

    want3, want_ids = gr.targets(gt_k, disp_k)
    want_seg = gr.as_prediction(seg_k, want3[:, 1:])
    t3, ids8, count = core.gt_instance_targets(gt, disp, segmentation=seg, return_key_count=True)
    t2, _ = core.gt_instance_targets(gt)
    torch.cuda.synchronize()
    same = (np.array_equal(t3[:k].cpu().numpy().view(np.uint32), want3.view(np.uint32)) and
            np.array_equal(t2[:k].cpu().numpy().view(np.uint32), want3[:, 1:].view(np.uint32)) and
            np.array_equal(ids8[:k].cpu().numpy(), want_ids) and np.array_equal(seg[:k].cpu().numpy(), want_seg) and
            (n < 2 * k or bool((t3[k:2 * k] == t3[:k]).all().item())))
    uniform = float((gt.view(n, rows // 8, 8, cols // 8, 8).amax((2, 4)) ==
                     gt.view(n, rows // 8, 8, cols // 8, 8).amin((2, 4))).float().mean().item())

    def timed(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(a.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts

    out2 = torch.empty_like(t2)
    out3 = torch.empty_like(t3)
    offsets = timed(lambda: core.gt_instance_targets(gt, segmentation=seg, out=out2))
    with_disp = timed(lambda: core.gt_instance_targets(gt, disp, segmentation=seg, out=out3))
    host_class = timed(lambda: st.GroundTruthOffsetsBatch(n, gt.data_ptr(), seg.data_ptr()))
    mode32 = timed(lambda: core.mode_downsample(gt))
    mode16 = timed(lambda: core.mode_downsample(disp))
    st.close()
    out = {"shape": [rows, cols], "n": n, "iters": a.iters, "identical": bool(same),
           "keys_per_frame_max": int(count.max().item()), "uniform_cells": round(uniform, 4),
           "targets2_ids_segmentation_ms_med_min_max": mmm(offsets),
           "targets3_ids_segmentation_ms_med_min_max": mmm(with_disp),
           "ground_truth_offsets_batch_ms_med_min_max": mmm(host_class),
           "mode_downsample_int32_ms_med_min_max": mmm(mode32),
           "mode_downsample_uint16_ms_med_min_max": mmm(mode16),
           "gt_bytes": 4 * n * rows * cols,
           "mode_downsample_int32_host_clock_TBps": round(4 * n * rows * cols / (min(mode32) * 1e-3) / 1e12, 3)}
    if not a.no_host:
        out.update(host_yardstick(a, gt_k, disp_k, n))
        fastest_host = min(v[1] for key, v in out.items() if key.startswith("host_restatement_"))
        out["yardstick_a_device_below_host"] = bool(max(with_disp) < fastest_host)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
