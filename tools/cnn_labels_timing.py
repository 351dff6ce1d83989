"""The CNN's own label maps of a batch and their confusion table in one launch (f15: is_cnn_label_maps,
core.cnn_label_maps) against the torch sequences it replaces, on the same device tensors (GPU box).

Prints one JSON line.  For cost planes [n][21][rows8][cols8] with 19 classes (default 64 x 21 x 128 x 256 -> images of
1024 x 2048), ms per batch by device events around the enqueued work, median of --iters (at least 10) after a warm-up,
with min and max, per mode ("nearest", "deconv") of
- the new call on preallocated outputs (one launch): label image + confusion table, the table alone (no d_label), the
  label image alone.  The ground truth is uniform noise per pixel, the worst case for the table (no two neighbouring
  pixels share a bin, so every pixel is one LDS add); `*_block_gt_*` repeats the two table timings on a ground truth of
  16 x 16 blocks, whose runs the kernel adds once each, as on real label images;
- the torch sequence: for "deconv" conv_transpose2d (groups = 19, the bilinear 16 x 16 weights, stride 8, padding 4)
  -> argmin -> table lookup -> bincount of gt * n_labels + pred; for "nearest" argmin -> repeat_interleave x 2 -> the
  same lookup and count.  The deconvolution's fp32 planes are 160 MB per frame, so that sequence runs in slices of
  --slice frames (default 8) whose tables are added; the timed window holds all slices;
- the copy yardstick: dst.copy_(src) of the two label images (gt and label), whose bytes read + written over its time
  is the copy bandwidth; `share_of_copy_bandwidth` is (gt read + label written + 19 planes read) over the new call's
  time, over that bandwidth.
`label_mismatch_vs_sequence` counts the pixels whose label differs from the torch sequence's (none in the nearest
mode; the library's transposed convolution sums in another order, so near-ties can differ in the other), and
`table_equal_to_sequence` compares the confusion tables.

    python tools/cnn_labels_timing.py [--n 64 --rows8 128 --cols8 256 --iters 20 --slice 8]
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
    ap.add_argument("--slice", type=int, default=8)
    a = ap.parse_args()
    if a.iters < 10:
        sys.exit("cnn_labels_timing.py: --iters must be at least 10")
    import numpy as np
    import torch
    import torch.nn.functional as F
    from instance_stixels_amd import core, evaluation
    if not torch.cuda.is_available():
        sys.exit("cnn_labels_timing.py needs a GPU")
    dev = torch.device("cuda", 0)
    n, Hs, Ws, NCLS, CH, NL = a.n, a.rows8, a.cols8, 19, 21, evaluation.CITYSCAPES_N_LABELS
    rows, cols = 8 * Hs, 8 * Ws
    torch.manual_seed(1)
    z = torch.randn((n, CH, Hs, Ws), device=dev)
    x = torch.cat((-F.log_softmax(3.0 * z[:, :NCLS], dim=1), z[:, NCLS:]), dim=1).contiguous()
    gt = torch.randint(0, NL, (n, rows, cols), dtype=torch.uint8, device=dev)
    table = torch.from_numpy(evaluation.CITYSCAPES_TRAINID_TO_LABELID.copy()).to(dev)
    k = torch.arange(16, device=dev)
    w1 = (2 * torch.minimum(k, 15 - k) + 1).float() / 16.0
    w2 = (w1[:, None] * w1[None, :]).expand(NCLS, 1, 16, 16).contiguous()
    stream = torch.cuda.current_stream(dev).cuda_stream
    label = torch.empty((n, rows, cols), dtype=torch.uint8, device=dev)
    conf = torch.zeros((NL, NL), dtype=torch.int64, device=dev)

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

    gt_blocks = torch.randint(0, NL, (n, rows // 16, cols // 16), dtype=torch.uint8, device=dev)
    gt_blocks = gt_blocks.repeat_interleave(16, dim=1).repeat_interleave(16, dim=2).contiguous()

    def call(mode, with_label, with_table, gt=gt):
        rc = core.cnn_label_maps_ptr(
            stream=stream, d_cnn_out=x.data_ptr(), n_images=n, channels=CH, n_classes=NCLS, rows8=Hs, cols8=Ws,
            mode=core.CNN_UP_MODES[mode], rows=rows, cols=cols, d_label=label.data_ptr() if with_label else None,
            d_gt_label=gt.data_ptr() if with_table else None, n_labels=NL if with_table else 0,
            d_confusion=conf.data_ptr() if with_table else None)
        assert rc == 0, core.lib().is_last_error()

    held = {}

    def count(pred, g):
        return torch.bincount(g.reshape(-1).long() * NL + pred.reshape(-1).long(), minlength=NL * NL)

    def sequence_nearest():
        idx = x[:, :NCLS].argmin(dim=1)
        idx = idx.repeat_interleave(8, dim=1).repeat_interleave(8, dim=2)
        held["label"] = table[idx]
        held["table"] = count(held["label"], gt)

    def sequence_deconv():
        total, labels = torch.zeros(NL * NL, dtype=torch.int64, device=dev), []
        for i in range(0, n, a.slice):
            up = F.conv_transpose2d(x[i:i + a.slice, :NCLS], w2, stride=8, padding=4, groups=NCLS)
            lab = table[up.argmin(dim=1)]
            total += count(lab, gt[i:i + a.slice])
            labels.append(lab)
        held["label"], held["table"] = torch.cat(labels), total

    src = torch.stack((gt, label))
    dst = torch.empty_like(src)
    t_copy = timed(lambda: dst.copy_(src))
    image_bytes = gt.numel()
    copy_bw = 2 * src.numel() / (float(np.median(t_copy)) * 1e-3)
    del src, dst
    plane_bytes = n * NCLS * Hs * Ws * 4
    out = {"shape": [n, CH, Hs, Ws], "image": [rows, cols], "classes": NCLS, "iters": a.iters, "slice": a.slice,
           "copy_ms_med_min_max": mmm(t_copy), "copy_bandwidth_GBps": round(copy_bw / 1e9, 1),
           "image_bytes": image_bytes, "plane_bytes": plane_bytes}
    for mode, sequence in (("nearest", sequence_nearest), ("deconv", sequence_deconv)):
        t_both = timed(lambda: call(mode, True, True))
        t_table = timed(lambda: call(mode, False, True))
        t_label = timed(lambda: call(mode, True, False))
        t_both_b = timed(lambda: call(mode, True, True, gt_blocks))
        t_table_b = timed(lambda: call(mode, False, True, gt_blocks))
        t_seq = timed(sequence)
        conf.zero_()
        call(mode, True, True)
        torch.cuda.synchronize()
        med = float(np.median(t_both))
        bw = (2 * image_bytes + plane_bytes) / (med * 1e-3)
        out[mode] = {
            "label_and_table_ms_med_min_max": mmm(t_both), "table_only_ms_med_min_max": mmm(t_table),
            "label_only_ms_med_min_max": mmm(t_label), "label_and_table_block_gt_ms_med_min_max": mmm(t_both_b),
            "table_only_block_gt_ms_med_min_max": mmm(t_table_b), "sequence_ms_med_min_max": mmm(t_seq),
            "call_GBps": round(bw / 1e9, 1), "share_of_copy_bandwidth": round(bw / copy_bw, 3),
            "faster_than_sequence": bool(med < float(np.median(t_seq))),
            "label_mismatch_vs_sequence": int((held["label"] != label).sum().item()), "pixels": label.numel(),
            "table_equal_to_sequence": bool(torch.equal(held["table"].view(NL, NL), conf)),
        }
        held.clear()
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
