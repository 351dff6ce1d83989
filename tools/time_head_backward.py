"""The backward pass of the segmentation head (f14: is_segmentation_head_backward, core.segmentation_head_backward)
against torch's autograd backward of the sequence it replaces, on the same device tensors (GPU box).

Prints one JSON line.  For fp32 and bf16 features [n][K][rows8][cols8] (default 64 x 512 x 128 x 256), ms per batch by
device events around the enqueued work, median of --iters (at least 10) after a warm-up, with min and max, of
- the new backward alone: core.segmentation_head_backward -> dX, dW, db (three launches);
- the same without dX (head-only fine-tuning: frozen features);
- the losses in front: is_semantic_nll and is_offset_loss write the class and the regression planes of one gy tensor
  in place (no memset, no copy), then the backward;
- the torch sequence: torch.autograd.grad of cat(-log_softmax(conv2d(x)[:, :19]), conv2d(x)[:, 19:]) with respect to
  x, weight and bias for the same gy (the forward graph is built once, outside the timing; the weights in the
  features' dtype);
- `max_abs_*_difference_vs_torch` compare the two results; `*dW_row0_max_abs_error_vs_float64` say which of the two
  is closer to a float64 evaluation of row 0 of dW on the call's own dz;
- the copy yardstick: dst.copy_(src) of the feature tensor; `backward_share_of_copy_bandwidth` is (feature bytes
  read + dX bytes written + 3 x the bytes of y) over the new call's time, over the copy's bandwidth.

    python tools/time_head_backward.py [--n 64 --K 512 --rows8 128 --cols8 256 --iters 20]
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
        sys.exit("time_head_backward.py: --iters must be at least 10")
    import numpy as np
    import torch
    import torch.nn.functional as F
    from instance_stixels_amd import core
    if not torch.cuda.is_available():
        sys.exit("time_head_backward.py needs a GPU")
    dev = torch.device("cuda", 0)
    n, K, Hs, Ws, NCLS, CH = a.n, a.K, a.rows8, a.cols8, 19, 21
    P = Hs * Ws
    torch.manual_seed(1)
    w = (torch.randn((CH, K), device=dev) * (2.0 / CH) ** 0.5).contiguous()
    b = (torch.randn((CH,), device=dev) * 0.1).contiguous()
    stream = torch.cuda.current_stream(dev).cuda_stream
    L = core.lib()
    rng = np.random.default_rng(2)
    target = rng.integers(0, NCLS, (n, Hs, Ws))
    target[rng.random((n, Hs, Ws)) < 0.1] = 255
    target = torch.tensor(target.astype(np.uint8), device=dev)
    # instances as 32 x 32 blocks of a checkerboard, stuff between them
    rows, cols = np.arange(Hs)[:, None] // 32, np.arange(Ws)[None, :] // 32
    ids = np.where((rows + cols) % 2 == 0, 26001 + rows * 64 + cols, 7).astype(np.int32)
    ids8 = torch.tensor(np.broadcast_to(ids, (n, Hs, Ws)).copy(), device=dev)
    loss1 = torch.empty((1,), dtype=torch.float32, device=dev)
    counts = torch.empty((2,), dtype=torch.int32, device=dev)
    loss5 = torch.empty((5,), dtype=torch.float32, device=dev)
    nll_scratch = torch.empty((core.semantic_nll_scratch_bytes(n, Hs, Ws),), dtype=torch.uint8, device=dev)
    off_bytes = core.offset_loss_scratch_bytes(n, 2, Hs, Ws)
    off_scratch = torch.empty((off_bytes,), dtype=torch.uint8, device=dev)

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

    def med(ts):
        return float(np.median(ts))

    out = {"shape": [n, K, Hs, Ws], "chunk": core.HEAD_BACKWARD_CHUNK, "iters": a.iters}
    for name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        x = torch.randn((n, K, Hs, Ws), device=dev).abs_().to(dtype).contiguous()
        y = core.segmentation_head(x, w, b, NCLS, 1 << Hs.bit_length(), want_segmentation=False)
        gy = torch.empty_like(y)

        def losses():
            rc = core.semantic_nll_ptr(
                stream, d_cnn_out=y.data_ptr(), cnn_image_stride=CH * P, d_target=target.data_ptr(),
                target_dtype=core.DTYPE_UINT8, ignore_index=255, n_images=n, rows8=Hs, cols8=Ws, n_classes=NCLS,
                d_loss=loss1.data_ptr(), d_valid_count=counts.data_ptr(), d_bad_count=counts.data_ptr() + 4,
                d_grad=gy.data_ptr(), grad_image_stride=CH * P, d_scratch=nll_scratch.data_ptr(),
                scratch_bytes=nll_scratch.numel())
            assert rc == 0, L.is_last_error()
            rc = core.offset_loss_ptr(
                stream, d_prediction=y.data_ptr() + 4 * NCLS * P, prediction_image_stride=CH * P,
                d_ids8=ids8.data_ptr(), n_images=n, planes=2, rows8=Hs, cols8=Ws, w_offset_mean=1e-3,
                w_offset_variance=1e-4, d_loss=loss5.data_ptr(), d_grad=gy.data_ptr() + 4 * NCLS * P,
                grad_image_stride=CH * P, d_scratch=off_scratch.data_ptr(), scratch_bytes=off_bytes)
            assert rc == 0, L.is_last_error()

        losses()
        held = {}

        def backward():
            held["g"] = core.segmentation_head_backward(x, w, y, gy, NCLS)

        def backward_frozen():
            held["f"] = core.segmentation_head_backward(x, w, y, gy, NCLS, want_features=False)

        def step():
            losses()
            backward()

        xt = x.detach().clone().requires_grad_(True)
        wd = w.to(dtype).reshape(CH, K, 1, 1).requires_grad_(True)
        bd = b.to(dtype).requires_grad_(True)
        z = F.conv2d(xt, wd, bd).float()
        seq_out = torch.cat((-F.log_softmax(z[:, :NCLS], dim=1), z[:, NCLS:]), dim=1)

        def sequence():
            held["s"] = torch.autograd.grad(seq_out, (xt, wd, bd), gy, retain_graph=True)

        def sequence_frozen():
            held["sf"] = torch.autograd.grad(seq_out, (wd, bd), gy, retain_graph=True)

        dst = torch.empty_like(x)
        t_bwd, t_frozen, t_step = timed(backward), timed(backward_frozen), timed(step)
        t_seq, t_seq_frozen = timed(sequence), timed(sequence_frozen)
        t_copy = timed(lambda: dst.copy_(x))
        feature_bytes = x.numel() * x.element_size()
        bwd_bytes = 2 * feature_bytes + 3 * y.numel() * 4
        copy_bw = 2 * feature_bytes / (med(t_copy) * 1e-3)
        bwd_bw = bwd_bytes / (med(t_bwd) * 1e-3)
        gs, g = held["s"], held["g"]
        # who is closer: row 0 of dW in float64 from the call's own dz, frame by frame
        dzv = core.segmentation_head_backward(x, w, y, gy, NCLS, want_features=False, want_weight=False,
                                              want_bias=False, want_logits=True)["logits"]
        row64 = torch.zeros((K,), dtype=torch.float64, device=dev)
        for i in range(n):
            row64 += x[i].reshape(K, P).double() @ dzv[i, 0].reshape(P).double()
        torch_dw = gs[1].float().reshape(CH, K)
        out[name] = {
            "backward_ms_med_min_max": mmm(t_bwd), "backward_without_dX_ms_med_min_max": mmm(t_frozen),
            "losses_and_backward_ms_med_min_max": mmm(t_step), "torch_backward_ms_med_min_max": mmm(t_seq),
            "torch_backward_without_dX_ms_med_min_max": mmm(t_seq_frozen), "copy_ms_med_min_max": mmm(t_copy),
            "feature_bytes": feature_bytes, "backward_bytes": bwd_bytes,
            "copy_bandwidth_GBps": round(copy_bw / 1e9, 1), "backward_GBps": round(bwd_bw / 1e9, 1),
            "backward_share_of_copy_bandwidth": round(bwd_bw / copy_bw, 3),
            "backward_faster_than_torch": bool(med(t_bwd) < med(t_seq)),
            "backward_without_dX_faster_than_torch": bool(med(t_frozen) < med(t_seq_frozen)),
            "max_abs_dW_difference_vs_torch": float((g["weight"] - torch_dw).abs().max().item()),
            "max_abs_dX_difference_vs_torch": float((g["features"].float() - gs[0].float()).abs().max().item()),
            "max_abs_dW": float(g["weight"].abs().max().item()),
            "max_abs_dX": float(g["features"].float().abs().max().item()),
            "dW_row0_max_abs_error_vs_float64": float((g["weight"][0].double() - row64).abs().max().item()),
            "torch_dW_row0_max_abs_error_vs_float64": float((torch_dw[0].double() - row64).abs().max().item()),
        }
        del x, xt, dst, y, gy, z, seq_out, held, gs, g, dzv, torch_dw
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
