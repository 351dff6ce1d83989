"""The offset and disparity training losses of a batch with their gradient on the device (f12: is_offset_loss,
core.offset_loss, training.DisparityOffsetLossSL; GPU box).

Prints one JSON line: ms per batch of n frames, host clock around the synchronised call, median of --iters after a
warm-up, with min and max, for
- core.offset_loss (3 planes, loss + terms + gradient, check=True: the key counts are read back);
- training.DisparityOffsetLossSL forward + loss.backward() into the leaf prediction;
- the yardstick: forward + backward of tests/offset_loss_reference.torch_loop_loss, the torch loop of the reference's
  structure, on the same device in float32, in the same process.
`done` is whether the fused call's SLOWEST run is below the yardstick's FASTEST run.  The fused result is checked
against the float64 restatement on the first frame before anything is timed.  The ids are instance_eval_reference.
synth_gt of the rendered instance image of synthetic frames, mode-downsampled by f11 (core.gt_instance_targets) with
the raw disparity; the prediction is f11's targets plus noise.  The kernels' own times come from a
`rocprofv3 --kernel-trace --stats` run of this script with --no-yardstick.

    python tools/offset_loss_timing.py [--rows 1024 --cols 2048 --max-dis 128 --n 8 --iters 20]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--cols", type=int, default=2048)
    ap.add_argument("--max-dis", type=int, default=128)
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--abs-variance", action="store_true")
    ap.add_argument("--no-yardstick", action="store_true", help="skip the torch loop: for runs under a profiler")
    a = ap.parse_args()
    import numpy as np
    import torch
    import helpers
    import instance_eval_reference as ir
    import offset_loss_reference as lr
    import render_reference as rr
    from instance_stixels_amd import core, host, synthetic, training
    if not torch.cuda.is_available():
        sys.exit("offset_loss_timing.py needs a GPU")
    rows, cols, D, n = a.rows, a.cols, a.max_dis, a.n
    dev = torch.device("cuda", 0)
    case = helpers.build_case("drn_d_22_unary", rows, cols, D, seed=1, n_images=1, size_filter=10)
    cfg = case["cfg"]
    frames = [synthetic.make_frame(cfg, seed=7 + i, n_slabs=12, offset_scale=1.0) for i in range(n)]
    big = torch.from_numpy(np.stack([f.disparity for f in frames])).to(dev)
    seg = torch.from_numpy(np.stack([f.segmentation for f in frames])).to(dev)
    road = [(f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground) for f in frames]
    st = host.Stixels()
    st.SetConfig(cfg)
    st.Initialize(max_batch=n)
    data, maps = st.ComputeBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), road, with_instances=True)
    st.close()
    secs = np.stack([d.sections for d in data])
    gt = np.clip(ir.synth_gt(rr.render(secs, rows, cols, maps)[2], seed=3), 0, 65535).astype(np.int32)
    disp = (np.clip(np.nan_to_num(np.stack([f.disparity for f in frames])), 0, 255) * 256).astype(np.uint16)
    disp[np.random.default_rng(5).random(disp.shape) < 0.04] = 0
    targets, ids8 = core.gt_instance_targets(torch.from_numpy(gt).to(dev), torch.from_numpy(disp).to(dev))
    d8 = core.mode_downsample(torch.from_numpy(disp).to(dev))
    torch.manual_seed(1)
    pred = (targets + torch.randn_like(targets) * torch.tensor([4.0, 1.5, 1.5], device=dev).view(1, 3, 1, 1)).contiguous()
    q = (d8.to(torch.int32) >> 8).float()
    weights = core.OFFSET_LOSS_WEIGHTS
    Hs, Ws = rows // 8, cols // 8
    torch.cuda.synchronize()

    loss5, terms, grad, count = core.offset_loss(pred, ids8, d8, weights=weights, abs_variance=a.abs_variance,
                                                 return_key_count=True)
    w32 = [float(np.float32(w)) for w in weights]
    want = lr.batch(pred[:1].cpu().numpy(), ids8[:1].cpu().numpy(), d8[:1].cpu().numpy(), w32, a.abs_variance)
    worst = max(float(lr.ulp_distance(terms[0].cpu().numpy(), want[1][0]).max()),
                float(lr.ulp_distance(grad[0].cpu().numpy(), want[2][0]).max()))

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

    fused = timed(lambda: core.offset_loss(pred, ids8, d8, weights=weights, abs_variance=a.abs_variance))
    unchecked = timed(lambda: core.offset_loss(pred, ids8, d8, weights=weights, abs_variance=a.abs_variance, check=False))
    fn = training.DisparityOffsetLossSL(abs_variance=a.abs_variance)
    leaf = pred.clone().requires_grad_(True)

    def module():
        leaf.grad = None
        fn(leaf, ids8, d8).backward()

    trained = timed(module)
    grad_bytes = n * Hs * Ws * (3 * 4 + 4 + 3 * 4)      # prediction and ids read, gradient written
    out = {"cells": [Hs, Ws], "n": n, "iters": a.iters, "abs_variance": bool(a.abs_variance),
           "keys_per_frame_max": int(count.max().item()), "frame0_max_ulp_vs_float64": round(worst, 3),
           "offset_loss_ms_med_min_max": mmm(fused), "offset_loss_unchecked_ms_med_min_max": mmm(unchecked),
           "training_forward_backward_ms_med_min_max": mmm(trained), "grad_pass_bytes": grad_bytes}
    if not a.no_yardstick:
        ids64 = ids8.long()

        def loop():
            leaf.grad = None
            lr.torch_loop_loss(leaf, ids64, q, weights, a.abs_variance)[0].backward()

        yard = timed(loop)
        loop_loss = float(lr.torch_loop_loss(pred, ids64, q, weights, a.abs_variance)[0])
        out["torch_loop_forward_backward_ms_med_min_max"] = mmm(yard, 1)
        out["torch_loop_loss"], out["offset_loss"] = loop_loss, float(loss5[0])
        out["done"] = bool(max(fused) < min(yard))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
