"""The backbone tail's layers in one launch each (f17: is_conv3x3_bn_relu, core.conv3x3_bn_relu) against the torch
sequence they replace, on the same device tensors (GPU box).

Prints one JSON line (progress on stderr).  For fp16 and bf16 features [n][C][rows8][cols8] (default 64 x 512 x 128 x
256) with half output, for dilation 2 (layer7) and 1 (layer8): ms per batch by device events around the enqueued work,
median of --iters (at least 10) with min and max, every arm of a (dtype, dilation) warmed up first and the arms then
ALTERNATING inside one loop, of
- the new call: core.conv3x3_bn_relu (one launch);
- the sequence, contiguous: F.conv2d + F.batch_norm (eval) + F.relu in the same dtype on NCHW tensors;
- the sequence, channels_last: the same on channels_last features and weights.
The faster of the two sequences is the comparison (`faster` is false where torch is as fast or faster: "not faster").
`tflop` is 2 * 9 * C * C * n * rows8 * cols8 from the shape; `mfma_floor_ms` is that over the dense half MFMA rate of
--cus compute units x 4 SIMDs x 1024 FLOP per clock at --mhz (take the clock from a counter run; the default is the
nominal 2400).  `dp_ints_differing` counts, on a batch of --dp-n frames, the DP input ints (core.segmentation_head of
the layer8 output of layer7) that differ between this path and the torch sequences in front of the same head.

    python tools/time_conv3x3.py [--n 64 --C 512 --rows8 128 --cols8 256 --iters 20 --mhz 2400 --cus 256 --dtypes fp16,bf16]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def mmm(ts, digits=3):
    import numpy as np
    return [round(float(np.median(ts)), digits), round(min(ts), digits), round(max(ts), digits)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--C", type=int, default=512)
    ap.add_argument("--rows8", type=int, default=128)
    ap.add_argument("--cols8", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--mhz", type=float, default=2400.0)
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--dp-n", type=int, default=0, help="0: the whole batch (a shape the library is already tuned for)")
    ap.add_argument("--dtypes", default="fp16,bf16", help="comma-separated subset of fp16,bf16")
    ap.add_argument("--no-torch", action="store_true", help="time the new call alone (for a counter run)")
    a = ap.parse_args()
    if a.iters < 10 and not a.no_torch:
        sys.exit("time_conv3x3.py: --iters must be at least 10")
    import numpy as np
    import torch
    import torch.nn.functional as F
    from instance_stixels_amd import core
    if not torch.cuda.is_available():
        sys.exit("time_conv3x3.py needs a GPU")
    dev = torch.device("cuda", 0)
    n, C, Hs, Ws = a.n, a.C, a.rows8, a.cols8
    P2S = 1 << Hs.bit_length()
    torch.manual_seed(1)
    w32 = torch.randn((C, C, 3, 3), device=dev) * (2.0 / (9 * C)) ** 0.5
    mean, var = torch.randn(C, device=dev) * 0.2, torch.rand(C, device=dev) + 0.5
    gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.1
    eps = 1e-5
    scale = (gamma.double() / torch.sqrt(var.double() + eps))
    shift = (beta.double() - mean.double() * scale).float()
    scale = scale.float()
    head_w = torch.randn((21, C), device=dev) * (2.0 / 21) ** 0.5
    head_b = torch.zeros(21, device=dev)
    tflop = 2.0 * 9 * C * C * n * Hs * Ws / 1e12
    floor_ms = tflop * 1e12 / (a.cus * 4 * 1024 * a.mhz * 1e6) * 1e3

    t_start = time.time()

    def note(*what):
        print("[%6.1f s]" % (time.time() - t_start), *what, file=sys.stderr, flush=True)

    def sequence(x, w, d, m, v, g, b):
        return F.relu(F.batch_norm(F.conv2d(x, w, padding=d, dilation=d), m, v, g, b, False, 0.0, eps))

    out = {"shape": [n, C, Hs, Ws], "iters": a.iters, "tflop_per_layer": round(tflop, 3), "mhz": a.mhz, "cus": a.cus,
           "mfma_floor_ms": round(floor_ms, 3)}
    for name, dtype in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        if name not in a.dtypes.split(","):
            continue
        x = torch.randn((n, C, Hs, Ws), device=dev).abs_().to(dtype).contiguous()
        packed = core.conv3x3_pack_weights(w32, dtype)
        wd = w32.to(dtype)
        bn = [t.to(dtype) for t in (mean, var, gamma, beta)]
        x_cl, w_cl = x.contiguous(memory_format=torch.channels_last), wd.contiguous(memory_format=torch.channels_last)
        for d in (2, 1):
            arms = {"new": lambda: core.conv3x3_bn_relu(x, packed, scale, shift, d)}
            if not a.no_torch:
                arms["torch_contiguous"] = lambda: sequence(x, wd, d, *bn)
                arms["torch_channels_last"] = lambda: sequence(x_cl, w_cl, d, *bn)
            for arm, fn in arms.items():            # warm-up of every arm (a library's first call may tune itself)
                note(name, "dilation", d, "warm-up", arm)
                for _ in range(2):
                    fn()
                torch.cuda.synchronize()
            ts = {arm: [] for arm in arms}
            for _ in range(a.iters):
                for arm, fn in arms.items():
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    fn()
                    t1.record()
                    t1.synchronize()
                    ts[arm].append(t0.elapsed_time(t1))
            med = {arm: float(np.median(t)) for arm, t in ts.items()}
            row = {arm + "_ms_med_min_max": mmm(t) for arm, t in ts.items()}
            row["new_tflops"] = round(tflop / (med["new"] * 1e-3), 1)
            row["new_share_of_mfma_floor"] = round(floor_ms / med["new"], 3)
            if not a.no_torch:
                best = min(med["torch_contiguous"], med["torch_channels_last"])
                row["torch_best_ms"] = round(best, 3)
                row["faster"] = bool(med["new"] < best)
            out["%s_d%d" % (name, d)] = row
            note(name, "dilation", d, json.dumps(row))
        if not a.no_torch:
            # the DP input of a small batch through both paths: layer7 (d = 2), layer8 (d = 1), the same head
            m = min(a.dp_n, n) if a.dp_n > 0 else n
            xs, xs_cl = x[:m].contiguous(), x_cl[:m]
            seg_new = core.segmentation_head(core.conv3x3_bn_relu(core.conv3x3_bn_relu(xs, packed, scale, shift, 2),
                                                                  packed, scale, shift, 1), head_w, head_b, 19, P2S)
            diff = {}
            for arm, (xx, ww) in (("torch_contiguous", (xs, wd)), ("torch_channels_last", (xs_cl, w_cl))):
                y = sequence(sequence(xx, ww, 2, *bn), ww, 1, *bn).contiguous()
                diff[arm] = int((core.segmentation_head(y, head_w, head_b, 19, P2S) != seg_new).sum().item())
            out[name + "_dp_ints_differing"] = dict(diff, ints=seg_new.numel(), frames=m)
        del x, x_cl, packed
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
