"""The full-resolution semantic NLL through the `up` layer (f16: is_semantic_nll_up, core.semantic_nll_up) against the
torch sequence it replaces, on the same device tensors (GPU box).

Prints one JSON line per shape.  For cost planes [n][21][rows8][cols8] with 19 classes (default 64 and 8 frames of
21 x 128 x 256 -> targets of 1024 x 2048), ms per batch by device events around the enqueued work, median of --iters
(at least 10) after a warm-up, with min and max, of
- the new call on preallocated outputs, as the loss alone (two launches) and as loss + gradient (three launches).
  The costs are -log_softmax of random logits; the ground truth is constant in 16 x 16 blocks with 10 % ignore_index;
- the torch sequence, forward and backward to the planes: conv_transpose2d (groups = 19, the bilinear 16 x 16 weights,
  stride 8, padding 4) of the negated planes -> log_softmax -> nll_loss(ignore_index, reduction='sum') / V.  Its fp32
  planes are 160 MB per frame and autograd keeps two of them, so it runs in slices of --slice frames (default 4)
  whose losses and gradients are added; the timed window holds all slices.  `sequence_forward_*` is the same without
  the backward (under no_grad);
- the copy yardstick: dst.copy_(src) of the call's compulsory bytes (the planes read, the targets read, the gradient
  written), whose bytes read + written over its time is the copy bandwidth; `share_of_copy_time` is that copy's time
  over the new call's.
`loss_diff_vs_sequence` and `grad_max_diff_vs_sequence` compare the two results (they sum in different orders).
Every step that uses the GPU is one process of this script under its own time limit:

    timeout -k 10 300 python tools/nll_up_timing.py --n 64
    timeout -k 10 300 python tools/nll_up_timing.py --n 8

    python tools/nll_up_timing.py [--n 64 --rows8 128 --cols8 256 --iters 20 --slice 4]
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
    ap.add_argument("--rows8", type=int, default=128)
    ap.add_argument("--cols8", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--slice", type=int, default=4)
    a = ap.parse_args()
    if a.iters < 10:
        sys.exit("nll_up_timing.py: --iters must be at least 10")
    import numpy as np
    import torch
    import torch.nn.functional as F
    from instance_stixels_amd import core
    if not torch.cuda.is_available():
        sys.exit("nll_up_timing.py needs a GPU")
    dev = torch.device("cuda", 0)
    n, Hs, Ws, NCLS, CH, IGNORE = a.n, a.rows8, a.cols8, 19, 21, 255
    rows, cols, P = 8 * Hs, 8 * Ws, Hs * Ws
    torch.manual_seed(1)
    z = torch.randn((n, CH, Hs, Ws), device=dev)
    x = torch.cat((-F.log_softmax(3.0 * z[:, :NCLS], dim=1), z[:, NCLS:]), dim=1).contiguous()
    tb = torch.randint(0, NCLS, (n, rows // 16, cols // 16), dtype=torch.uint8, device=dev)
    tb[torch.rand(tb.shape, device=dev) < 0.1] = IGNORE
    target = tb.repeat_interleave(16, dim=1).repeat_interleave(16, dim=2).contiguous()
    k = torch.arange(16, device=dev)
    w1 = (2 * torch.minimum(k, 15 - k) + 1).float() / 16.0
    w2 = (w1[:, None] * w1[None, :]).expand(NCLS, 1, 16, 16).contiguous()
    stream = torch.cuda.current_stream(dev).cuda_stream
    loss = torch.empty(1, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    grad = torch.empty((n, NCLS, Hs, Ws), device=dev)
    nbytes = core.semantic_nll_up_scratch_bytes(n, Hs, Ws, NCLS)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)

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

    def call(with_grad):
        rc = core.semantic_nll_up_ptr(
            stream=stream, d_cnn_out=x.data_ptr(), cnn_image_stride=CH * P, d_target=target.data_ptr(),
            ignore_index=IGNORE, n_images=n, rows8=Hs, cols8=Ws, n_classes=NCLS, mode=core.CNN_UP_DECONV, rows=rows,
            cols=cols, d_loss=loss.data_ptr(), d_valid_count=counts.data_ptr(), d_bad_count=counts.data_ptr() + 8,
            d_grad=grad.data_ptr() if with_grad else None, grad_image_stride=NCLS * P, d_scratch=scratch.data_ptr(),
            scratch_bytes=nbytes)
        assert rc == 0, core.lib().is_last_error()

    held = {}
    valid = (target != IGNORE).sum()

    def sequence(backward):
        total = torch.zeros((), device=dev)
        grads = []
        for i in range(0, n, a.slice):
            y = x[i:i + a.slice, :NCLS].detach().requires_grad_(backward)
            up = F.conv_transpose2d(-y, w2, stride=8, padding=4, groups=NCLS)
            part = F.nll_loss(F.log_softmax(up, dim=1), target[i:i + a.slice].long(), ignore_index=IGNORE,
                              reduction="sum") / valid
            if backward:
                part.backward()
                grads.append(y.grad)
            total += part.detach()
        held["loss"] = total
        if backward:
            held["grad"] = torch.cat(grads)

    def forward_only():
        with torch.no_grad():
            sequence(False)

    src = torch.empty(n * NCLS * P * 4 + target.numel(), dtype=torch.uint8, device=dev)   # planes + targets
    dst = torch.empty_like(src)
    t_copy = timed(lambda: dst.copy_(src))
    copy_bw = 2 * src.numel() / (float(np.median(t_copy)) * 1e-3)
    # the compulsory bytes of loss + gradient: planes and targets read, the gradient written
    compulsory = src.numel() + n * NCLS * P * 4
    del src, dst
    t_loss = timed(lambda: call(False))
    t_both = timed(lambda: call(True))
    t_fwd = timed(forward_only)
    t_seq = timed(lambda: sequence(True))
    call(True)
    torch.cuda.synchronize()
    med_loss, med_both = float(np.median(t_loss)), float(np.median(t_both))
    copy_ms = compulsory / copy_bw * 1e3
    out = {
        "shape": [n, CH, Hs, Ws], "target": [rows, cols], "classes": NCLS, "iters": a.iters, "slice": a.slice,
        "copy_ms_med_min_max": mmm(t_copy), "copy_bandwidth_GBps": round(copy_bw / 1e9, 1),
        "compulsory_bytes": compulsory, "compulsory_copy_ms": round(copy_ms, 3),
        "loss_only_ms_med_min_max": mmm(t_loss), "loss_and_grad_ms_med_min_max": mmm(t_both),
        "sequence_forward_ms_med_min_max": mmm(t_fwd), "sequence_ms_med_min_max": mmm(t_seq),
        "share_of_copy_time": round(copy_ms / med_both, 4),
        "loss_only_faster_than_sequence_forward": bool(med_loss < float(np.median(t_fwd))),
        "loss_and_grad_faster_than_sequence": bool(med_both < float(np.median(t_seq))),
        "valid": int(counts[0].item()), "bad": int(counts[1].item()), "valid_of_sequence": int(valid.item()),
        "loss": float(loss.item()), "loss_diff_vs_sequence": abs(float(loss.item()) - float(held["loss"].item())),
        "grad_max_diff_vs_sequence": float((held["grad"] - grad).abs().max().item()),
        "grad_max_abs": float(grad.abs().max().item()),
    }
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
