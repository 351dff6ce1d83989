"""The CNN's segmentation head of a batch in one launch (f13: is_segmentation_head, core.segmentation_head) against
the sequence it replaces, on the same device tensors (GPU box).

Prints one JSON line.  For fp32 and bf16 features [n][K][rows8][cols8] (default 64 x 512 x 128 x 256), ms per batch by
device events around the enqueued work, median of --iters (at least 10) after a warm-up, with min and max, of
- the new call: core.segmentation_head -> the DP's int32 tensor (one launch);
- the sequence: torch.nn.functional.conv2d (1x1, the weights in the features' dtype, the result widened to fp32),
  log_softmax over the 19 class channels, negation and cat with the 2 offset channels, is_flip_and_pad;
- the copy yardstick: dst.copy_(src) of the feature tensor, whose bytes read + written over its time is the copy
  bandwidth; `head_share_of_copy_bandwidth` is (feature bytes + weight bytes + int32 bytes written) over the new
  call's time, over that bandwidth.
`int_mismatch_vs_sequence` counts the DP inputs in which the two differ (the library convolution sums in another
order; the new call is the k-ordered fmaf chain of the contract, which tests/test_segmentation_head_gpu.py pins).

    python tools/time_head.py [--n 64 --K 512 --rows8 128 --cols8 256 --iters 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def mmm(ts, digits=3):
    import numpy as np
    return [round(float(np.median(ts)), digits), round(min(ts), digits), round(max(ts), digits)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--K", type=int, default=512)
    ap.add_argument("--rows8", type=int, default=128)
    ap.add_argument("--cols8", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if a.iters < 10:
        sys.exit("time_head.py: --iters must be at least 10")
    import torch
    import torch.nn.functional as F
    from instance_stixels_amd import core
    if not torch.cuda.is_available():
        sys.exit("time_head.py needs a GPU")
    dev = torch.device("cuda", 0)
    n, K, Hs, Ws, NCLS, CH = a.n, a.K, a.rows8, a.cols8, 19, 21
    P2S = 1 << Hs.bit_length()          # the power of two >= rows8 + 1
    torch.manual_seed(1)
    w = (torch.randn((CH, K), device=dev) * (2.0 / CH) ** 0.5).contiguous()
    b = (torch.randn((CH,), device=dev) * 0.1).contiguous()
    stream = torch.cuda.current_stream(dev).cuda_stream
    L = core.lib()

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.iters):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            ts.append(t0.elapsed_time(t1))
        return ts

    out = {"shape": [n, K, Hs, Ws], "P2S": P2S, "iters": a.iters}
    for name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        x = torch.randn((n, K, Hs, Ws), device=dev).abs_().to(dtype).contiguous()
        wd, bd = w.to(dtype).reshape(CH, K, 1, 1), b.to(dtype)
        seg_seq = torch.empty((n, Ws, CH, P2S), dtype=torch.int32, device=dev)
        held = {}

        def head():
            held["seg"] = core.segmentation_head(x, w, b, NCLS, P2S)

        def sequence():
            y = F.conv2d(x, wd, bd).float()
            cnn = torch.cat((-F.log_softmax(y[:, :NCLS], dim=1), y[:, NCLS:]), dim=1)
            rc = L.is_flip_and_pad(cnn.data_ptr(), seg_seq.data_ptr(), n, CH, Hs, Ws, P2S, stream)
            assert rc == 0, L.is_last_error()

        dst = torch.empty_like(x)
        t_head, t_seq = timed(head), timed(sequence)
        t_copy = timed(lambda: dst.copy_(x))
        feature_bytes = x.numel() * x.element_size()
        head_bytes = feature_bytes + (w.numel() + b.numel()) * 4 + seg_seq.numel() * 4
        copy_bw = 2 * feature_bytes / (float(torch.tensor(t_copy).median()) * 1e-3)
        head_bw = head_bytes / (float(torch.tensor(t_head).median()) * 1e-3)
        out[name] = {
            "head_ms_med_min_max": mmm(t_head), "sequence_ms_med_min_max": mmm(t_seq),
            "copy_ms_med_min_max": mmm(t_copy), "feature_bytes": feature_bytes, "head_bytes": head_bytes,
            "copy_bandwidth_GBps": round(copy_bw / 1e9, 1), "head_GBps": round(head_bw / 1e9, 1),
            "head_share_of_copy_bandwidth": round(head_bw / copy_bw, 3),
            "head_faster_than_sequence": bool(float(torch.tensor(t_head).median()) < float(torch.tensor(t_seq).median())),
            "int_mismatch_vs_sequence": int((held["seg"] != seg_seq).sum().item()), "ints": seg_seq.numel(),
        }
        del x, dst, seg_seq, held
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
