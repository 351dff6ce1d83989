"""The backbone's convolutions on the device (f17: is_conv3x3_bn_relu, core.conv3x3_bn_relu; f18: is_conv_bn,
core.conv_bn, cnn.ResidualBlock; f19: is_conv_bn_stride, core.conv_bn_stride, cnn.StridedResidualBlock; f20: is_stem, core.stem) against what
they replace and against themselves, on the same device tensors (GPU
box).

Prints one JSON line (progress on stderr).  Every timing is ms per batch by device events around the enqueued work,
median of --iters (at least 10) with min and max, every arm of a comparison warmed up first and the arms then
ALTERNATING inside one loop.  The torch arms are the same work in the same dtype on contiguous (NCHW) and on
channels_last tensors; the faster of the two is the comparison (`faster` is false where torch is as fast or faster:
"not faster").  `mfma_floor_ms` is a part's FLOP over the dense half MFMA rate of --cus compute units x 4 SIMDs x 1024
FLOP per clock at --mhz (take the clock from a counter run; the default is the nominal 2400).  Parts (--parts,
comma-separated), for fp16 and bf16 features [n][.][rows8][cols8] with half output:
- tail: core.conv3x3_bn_relu (one launch, --C channels) for dilation 2 (layer7) and 1 (layer8) against F.conv2d +
  F.batch_norm (eval) + F.relu.  `dp_ints_differing` counts, on a batch of --dp-n frames, the DP input ints
  (core.segmentation_head of the layer8 output of layer7) that differ between this path and the torch sequences in
  front of the same head.
- residual: core.conv_bn (3x3, dilation 2, --C channels) with a residual operand against the same call without one;
  `residual_gb` is the extra operand's bytes.
- 1x1: the downsample launch (core.conv_bn, kernel 1, no ReLU) at 128 -> 256 and 256 -> 512 channels against F.conv2d +
  F.batch_norm (eval).
- layers: layer5 + layer6 of drn_d_22 (two BasicBlocks each, 128 -> 256 -> 512, dilations 2 and 4, the first block of
  each with a downsample) through cnn.ResidualBlock (10 launches) against the torch modules.
- strided (not in the default --parts): the downsampling layers of drn_d_22 on layer1's output [n][16][--rows][--cols]
  in half: each distinct new launch shape -- 3x3 stride 2 at 16 -> 32, 32 -> 64 and 64 -> 128, 1x1 stride 2 at 32 -> 64
  and 64 -> 128, 3x3 stride 1 with a residual at 64 and 128 channels, each at its layer's resolution -- against
  F.conv2d(stride) + F.batch_norm (+ residual) (+ F.relu), and layer2 + layer3 + layer4 whole (11 launches) against the
  torch modules.  --strided-n frames per call (default --n): a slice of the batch where torch's intermediates or its
  warm-up are too large; the row says how many.
- stem (not in the default --parts): core.stem on the camera's bytes [n][--rows][--cols][3], with and without d_mid,
  against torch's sequence on the same bytes: byte -> float / 255 -> normalise -> half -> conv2d 7x7 -> batch_norm ->
  relu -> conv2d 3x3 -> batch_norm -> relu.  `compulsory_gb` is 3 + 32 bytes per pixel.  --stem-n frames per call
  (default --n) where torch's intermediates or its warm-up are too large; the row says how many.
- backward (not in the default --parts): core.conv_bn_backward (f21) with every gradient (dX, dW, dscale, dshift) and
  without dX, at --backward-n frames (default 4, the size training uses): 3x3 at --C channels with dilation 2 and 1
  (layer7, layer8), and layer5's and layer6's pairs 128 -> 256 (dilation 2) and 256 -> 512 (dilation 4) as 3x3 and as
  1x1, against torch.autograd.grad of relu(batch_norm_eval(conv2d(x))) in the same half dtype with respect to x, the
  weight and the BatchNorm affine pair, the forward graph built outside the timing.  `scratch_mb` is the call's scratch.
  The MFMA floor counts dX and dW: 2 x the forward's FLOP.  Both arms allocate their outputs inside the timing (torch's
  caching allocator; the library's arm also its scratch), as a training step does.  --backward-cases picks shapes.
- stem_backward (not in the default --parts): core.stem_backward (f23) on --stem-n frames of [--rows][--cols][3] bytes
  with every gradient, from dY (`new`) and from layer2's masked gradient at 32 channels (`new_next`), against
  torch.autograd.grad of the same three layers (and, for `_next`, of layer2's convolution on top) in the same half
  dtype.  `compulsory_gb` is 3 + 32 + 32 + 32 bytes per pixel: the image, dY, out and mid once each.
- backward_stride (not in the default --parts): core.conv_bn_stride_backward (f22) at the five stride-2 launches of
  drn_d_22 on layer1's output [--backward-n][16][--rows][--cols] -- 3x3 at 16 -> 32 (layer2, no dX: it is refused at 16
  channels), 32 -> 64 and 64 -> 128, 1x1 at 32 -> 64 and 64 -> 128, each at its layer's resolution -- with every gradient
  and without dX, against torch.autograd.grad as in `backward` (with respect to x too, except at layer2).
  `compulsory_gb` is x, the saved output (3x3), dY and dX once each; `new_share_of_hbm_floor` is its time at --hbm-gbs
  over the call's.  --backward-stride-cases picks launches.
--no-torch leaves the torch arms out (and alone allows fewer than 10 iterations, for a counter run).  torch's first
convolution of a shape takes 30 - 160 s: run the dtypes, and if need be the parts, in separate commands.

    python tools/time_conv.py [--n 64 --C 512 --rows8 128 --cols8 256 --iters 20 --mhz 2400 --cus 256 --dtypes fp16,bf16
                               --parts tail,residual,1x1,layers[,strided][,stem][,backward][,backward_stride][,stem_backward] --rows 1024 --cols 2048 --strided-n 64
                               --stem-n 64
                               --no-torch]
"""
import argparse
import copy
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
    ap.add_argument("--C", type=int, default=512, help="channels of the `tail` and `residual` parts")
    ap.add_argument("--rows8", type=int, default=128)
    ap.add_argument("--cols8", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--mhz", type=float, default=2400.0)
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--dp-n", type=int, default=0, help="0: the whole batch (a shape the library is already tuned for)")
    ap.add_argument("--dtypes", default="fp16,bf16", help="comma-separated subset of fp16,bf16")
    ap.add_argument("--parts", default="tail,residual,1x1,layers",
                    help="comma-separated subset of tail,residual,1x1,layers,strided,stem,backward,backward_stride,stem_backward")
    ap.add_argument("--backward-stride-cases", default="0,1,2,3,4", help="which of the five launches of `backward_stride`")
    ap.add_argument("--hbm-gbs", type=float, default=6300.0, help="the memory rate of the compulsory-traffic floor")
    ap.add_argument("--backward-n", type=int, default=4, help="frames per call of the `backward` part")
    ap.add_argument("--backward-cases", default="0,1,2,3,4,5", help="which of the six shapes of the `backward` part")
    ap.add_argument("--rows", type=int, default=1024, help="rows of layer1's output (the `strided` part)")
    ap.add_argument("--cols", type=int, default=2048)
    ap.add_argument("--strided-n", type=int, default=0, help="frames per call of the `strided` part; 0: --n")
    ap.add_argument("--stem-n", type=int, default=0, help="frames per call of the `stem` part; 0: --n")
    ap.add_argument("--no-torch", action="store_true", help="time the library's launches alone")
    a = ap.parse_args()
    if a.iters < 10 and not a.no_torch:
        sys.exit("time_conv.py: --iters must be at least 10")
    import numpy as np
    import torch
    import torch.nn.functional as F
    from instance_stixels_amd import cnn, core
    if not torch.cuda.is_available():
        sys.exit("time_conv.py needs a GPU")
    dev = torch.device("cuda", 0)
    n, Hs, Ws = a.n, a.rows8, a.cols8
    parts = a.parts.split(",")
    torch.manual_seed(1)
    eps = 1e-5
    t_start = time.time()

    def note(*what):
        print("[%6.1f s]" % (time.time() - t_start), *what, file=sys.stderr, flush=True)

    def floor_ms(tflop):
        return tflop * 1e12 / (a.cus * 4 * 1024 * a.mhz * 1e6) * 1e3

    def bn_stats(c):
        return (torch.randn(c, device=dev) * 0.2, torch.rand(c, device=dev) + 0.5, torch.rand(c, device=dev) + 0.5,
                torch.randn(c, device=dev) * 0.1)                              # mean, var, gamma, beta

    def fold(mean, var, gamma, beta):
        scale = gamma.double() / torch.sqrt(var.double() + eps)
        return scale.float(), (beta.double() - mean.double() * scale).float()

    def weight(cout, cin, k):
        return torch.randn((cout, cin, k, k), device=dev) * (2.0 / (k * k * cout)) ** 0.5

    def torch_conv_bn(x, w, d, bn, relu, stride=1, residual=None):
        y = F.batch_norm(F.conv2d(x, w, stride=stride, padding=d * (w.shape[2] // 2), dilation=d), *bn, False, 0.0, eps)
        if residual is not None:
            y = y + residual
        return F.relu(y) if relu else y

    def channels_last(*ts):
        return [t.contiguous(memory_format=torch.channels_last) for t in ts]

    def measure(label, arms):
        for arm, fn in arms.items():                # warm-up of every arm (a library's first call may tune itself)
            note(label, "warm-up", arm)
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
        row = {arm + "_ms_med_min_max": mmm(t) for arm, t in ts.items()}
        return row, {arm: float(np.median(t)) for arm, t in ts.items()}

    def against_torch(row, med, new="new"):
        if not a.no_torch:
            best = min(med["torch_contiguous"], med["torch_channels_last"])
            row["torch_best_ms"] = round(best, 3)
            row["new_over_torch_best"] = round(med[new] / best, 3)
            row["faster"] = bool(med[new] < best)

    class TorchBlock(torch.nn.Module):
        """conv1, bn1, relu, conv2, bn2, (+ downsample(x) or x), relu: a BasicBlock in eval mode."""

        def __init__(self, cin, cout, d, dtype, stride=1):
            super().__init__()
            self.conv1 = torch.nn.Conv2d(cin, cout, 3, stride=stride, padding=d, dilation=d, bias=False)
            self.bn1 = torch.nn.BatchNorm2d(cout)
            self.conv2 = torch.nn.Conv2d(cout, cout, 3, padding=d, dilation=d, bias=False)
            self.bn2 = torch.nn.BatchNorm2d(cout)
            self.downsample = None
            if cin != cout:
                self.downsample = torch.nn.Sequential(torch.nn.Conv2d(cin, cout, 1, stride=stride, bias=False),
                                                      torch.nn.BatchNorm2d(cout))
            self.residual = True
            with torch.no_grad():
                for m in self.modules():
                    if isinstance(m, torch.nn.Conv2d):
                        m.weight.copy_(weight(m.out_channels, m.in_channels, m.kernel_size[0]))
                    elif isinstance(m, torch.nn.BatchNorm2d):
                        mean, var, gamma, beta = bn_stats(m.num_features)
                        m.running_mean.copy_(mean), m.running_var.copy_(var), m.weight.copy_(gamma), m.bias.copy_(beta)
            self.eval()

        def forward(self, x):
            out = self.bn2(self.conv2(F.relu(self.bn1(self.conv1(x)))))
            out = out + (x if self.downsample is None else self.downsample(x))
            return F.relu(out)

    out = {"frames": n, "plane": [Hs, Ws], "iters": a.iters, "mhz": a.mhz, "cus": a.cus}
    for name, dtype in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        if name not in a.dtypes.split(","):
            continue
        if "tail" in parts:
            C = a.C
            tflop = 2.0 * 9 * C * C * n * Hs * Ws / 1e12
            out.update(shape=[n, C, Hs, Ws], tflop_per_layer=round(tflop, 3), mfma_floor_ms=round(floor_ms(tflop), 3))
            x = torch.randn((n, C, Hs, Ws), device=dev).abs_().to(dtype).contiguous()
            w32, stats = weight(C, C, 3), bn_stats(C)
            packed, (scale, shift) = core.conv3x3_pack_weights(w32, dtype), fold(*stats)
            if not a.no_torch:
                wd, bn = w32.to(dtype), [t.to(dtype) for t in stats]
                x_cl, w_cl = channels_last(x, wd)
            for d in (2, 1):
                arms = {"new": lambda: core.conv3x3_bn_relu(x, packed, scale, shift, d)}
                if not a.no_torch:
                    arms["torch_contiguous"] = lambda: torch_conv_bn(x, wd, d, bn, True)
                    arms["torch_channels_last"] = lambda: torch_conv_bn(x_cl, w_cl, d, bn, True)
                row, med = measure("%s dilation %d" % (name, d), arms)
                row.update(new_tflops=round(tflop / (med["new"] * 1e-3), 1),
                           new_share_of_mfma_floor=round(floor_ms(tflop) / med["new"], 3))
                against_torch(row, med)
                out["%s_d%d" % (name, d)] = row
                note(name, "dilation", d, json.dumps(row))
            if not a.no_torch:
                # the DP input of a small batch through both paths: layer7 (d = 2), layer8 (d = 1), the same head
                m = min(a.dp_n, n) if a.dp_n > 0 else n
                P2S = 1 << Hs.bit_length()
                head_w, head_b = torch.randn((21, C), device=dev) * (2.0 / 21) ** 0.5, torch.zeros(21, device=dev)
                xs, xs_cl = x[:m].contiguous(), x_cl[:m]
                seg_new = core.segmentation_head(core.conv3x3_bn_relu(core.conv3x3_bn_relu(xs, packed, scale, shift, 2),
                                                                      packed, scale, shift, 1), head_w, head_b, 19, P2S)
                diff = {}
                for arm, (xx, ww) in (("torch_contiguous", (xs, wd)), ("torch_channels_last", (xs_cl, w_cl))):
                    y = torch_conv_bn(torch_conv_bn(xx, ww, 2, bn, True), ww, 1, bn, True).contiguous()
                    diff[arm] = int((core.segmentation_head(y, head_w, head_b, 19, P2S) != seg_new).sum().item())
                out[name + "_dp_ints_differing"] = dict(diff, ints=seg_new.numel(), frames=m)
                del x_cl
            del x, packed
            torch.cuda.empty_cache()
        if "residual" in parts:
            C = a.C
            x = torch.randn((n, C, Hs, Ws), device=dev).abs_().to(dtype)
            res = torch.randn((n, C, Hs, Ws), device=dev).to(dtype)
            packed, (scale, shift) = core.conv_pack_weights(weight(C, C, 3), dtype), fold(*bn_stats(C))
            tflop = 2.0 * 9 * C * C * n * Hs * Ws / 1e12
            row, med = measure(name + " residual", {
                "plain": lambda: core.conv_bn(x, packed, scale, shift, 3, 2),
                "residual": lambda: core.conv_bn(x, packed, scale, shift, 3, 2, residual=res),
                "residual_is_features": lambda: core.conv_bn(x, packed, scale, shift, 3, 2, residual=x)})
            row.update(shape=[n, C, Hs, Ws], residual_gb=round(res.numel() * 2 / 1e9, 3),
                       residual_minus_plain_ms=round(med["residual"] - med["plain"], 3),
                       residual_tflops=round(tflop / (med["residual"] * 1e-3), 1))
            out[name + "_residual"] = row
            note(name, "residual", json.dumps(row))
            del x, res, packed
            torch.cuda.empty_cache()
        if "1x1" in parts:
            for cin, cout in ((128, 256), (256, 512)):
                x = torch.randn((n, cin, Hs, Ws), device=dev).abs_().to(dtype)
                w32, stats = weight(cout, cin, 1), bn_stats(cout)
                packed, (scale, shift) = core.conv_pack_weights(w32, dtype), fold(*stats)
                arms = {"new": lambda: core.conv_bn(x, packed, scale, shift, 1, relu=False)}
                if not a.no_torch:
                    wd, bn = w32.to(dtype), [t.to(dtype) for t in stats]
                    x_cl, w_cl = channels_last(x, wd)
                    arms["torch_contiguous"] = lambda: torch_conv_bn(x, wd, 1, bn, False)
                    arms["torch_channels_last"] = lambda: torch_conv_bn(x_cl, w_cl, 1, bn, False)
                row, med = measure("%s 1x1 %d->%d" % (name, cin, cout), arms)
                gb = n * Hs * Ws * (cin + cout) * 2 / 1e9
                row.update(compulsory_gb=round(gb, 3), new_gb_per_s=round(gb / (med["new"] * 1e-3), 1),
                           new_tflops=round(2.0 * cin * cout * n * Hs * Ws / 1e12 / (med["new"] * 1e-3), 1))
                against_torch(row, med)
                out["%s_1x1_%d_%d" % (name, cin, cout)] = row
                note(name, "1x1", cin, cout, json.dumps(row))
                del x, packed
                if not a.no_torch:
                    del x_cl
                torch.cuda.empty_cache()
        if "layers" in parts:
            blocks = [TorchBlock(128, 256, 2, dtype), TorchBlock(256, 256, 2, dtype), TorchBlock(256, 512, 4, dtype),
                      TorchBlock(512, 512, 4, dtype)]
            ours = [cnn.ResidualBlock(b.to(dev), dtype=dtype) for b in blocks]      # (folded from the fp32 modules)
            macs = sum(m.weight.numel() for b in blocks for m in b.modules() if isinstance(m, torch.nn.Conv2d))
            tflop = 2.0 * macs * n * Hs * Ws / 1e12
            x = torch.randn((n, 128, Hs, Ws), device=dev).abs_().to(dtype)

            def new():
                y = x
                for blk in ours:
                    y = blk(y)
                return y
            arms = {"new": new}
            if not a.no_torch:
                seq = torch.nn.Sequential(*blocks).to(device=dev, dtype=dtype).eval()
                seq_cl = copy.deepcopy(seq).to(memory_format=torch.channels_last).eval()
                x_cl, = channels_last(x)
                arms["torch_contiguous"] = lambda: seq(x)
                arms["torch_channels_last"] = lambda: seq_cl(x_cl)
            with torch.no_grad():
                row, med = measure(name + " layer5+layer6", arms)
            row.update(shape_in=[n, 128, Hs, Ws], launches=10, tflop=round(tflop, 3),
                       mfma_floor_ms=round(floor_ms(tflop), 3), new_tflops=round(tflop / (med["new"] * 1e-3), 1),
                       new_share_of_mfma_floor=round(floor_ms(tflop) / med["new"], 3))
            against_torch(row, med)
            out[name + "_layers"] = row
            note(name, "layers", json.dumps(row))
            del x, ours
            torch.cuda.empty_cache()
        if "backward" in parts:
            m = a.backward_n
            cases = ((a.C, a.C, 3, 2), (a.C, a.C, 3, 1), (128, 256, 3, 2), (128, 256, 1, 1), (256, 512, 3, 4), (256, 512, 1, 1))
            for cin, cout, k, d in [cases[int(i)] for i in a.backward_cases.split(",")]:
                relu = k == 3                                                  # (the 1x1 is the downsample: no ReLU)
                x = torch.randn((m, cin, Hs, Ws), device=dev).abs_().to(dtype)
                w32, stats = weight(cout, cin, k), bn_stats(cout)
                scale, shift = fold(*stats)
                y = core.conv_bn(x, core.conv_pack_weights(w32, dtype), scale, shift, k, d, relu=relu)
                gy = torch.randn((m, cout, Hs, Ws), device=dev).to(dtype)
                arms = {"new": lambda: core.conv_bn_backward(x, w32, scale, y, gy, k, d, relu=relu),
                        "new_no_dx": lambda: core.conv_bn_backward(x, w32, scale, y, gy, k, d, relu=relu,
                                                                   want_features=False)}
                if not a.no_torch:
                    graphs = {}
                    for arm, cl in (("torch_contiguous", False), ("torch_channels_last", True)):
                        xt, wt = x.clone(), w32.to(dtype)
                        if cl:
                            xt, wt = channels_last(xt, wt)
                        xt, wt = xt.requires_grad_(True), wt.requires_grad_(True)
                        mean, var, gamma, beta = [t.to(dtype) for t in stats]
                        gamma, beta = gamma.requires_grad_(True), beta.requires_grad_(True)
                        yt = F.batch_norm(F.conv2d(xt, wt, padding=d * (k // 2), dilation=d), mean, var, gamma, beta, False,
                                          0.0, eps)
                        yt = F.relu(yt) if relu else yt
                        graphs[arm] = (yt, (xt, wt, gamma, beta), channels_last(gy)[0] if cl else gy)
                        arms[arm] = lambda arm=arm: torch.autograd.grad(graphs[arm][0], graphs[arm][1], graphs[arm][2],
                                                                        retain_graph=True)
                row, med = measure("%s backward %d->%d k%d d%d" % (name, cin, cout, k, d), arms)
                tflop = 2 * 2.0 * k * k * cin * cout * m * Hs * Ws / 1e12
                row.update(shape=[m, cin, cout, Hs, Ws, k, d], tflop=round(tflop, 3), mfma_floor_ms=round(floor_ms(tflop), 3),
                           new_share_of_mfma_floor=round(floor_ms(tflop) / med["new"], 3),
                           scratch_mb=round(core.conv_bn_backward_scratch_bytes(
                               m, cin, cout, Hs, Ws, k, core.HEAD_F16 if dtype == torch.float16 else core.HEAD_BF16) / 2 ** 20, 1))
                against_torch(row, med)
                out["%s_backward_%d_%d_k%d_d%d" % (name, cin, cout, k, d)] = row
                note(name, "backward", json.dumps(row))
                del x, y, gy, arms
                if not a.no_torch:
                    del graphs
                torch.cuda.empty_cache()
        if "backward_stride" in parts:
            m, H1, W1 = a.backward_n, a.rows, a.cols
            half = lambda v, times: -(-v // 2 ** times)                      # ceil(v / 2^times)
            # (label, channels_in, channels_out, kernel, level of the input's resolution)
            cases = (("3x3s2_16_32", 16, 32, 3, 0), ("3x3s2_32_64", 32, 64, 3, 1), ("1x1s2_32_64", 32, 64, 1, 1),
                     ("3x3s2_64_128", 64, 128, 3, 2), ("1x1s2_64_128", 64, 128, 1, 2))
            for label, cin, cout, k, level in [cases[int(i)] for i in a.backward_stride_cases.split(",")]:
                relu, dx = k == 3, cin % 32 == 0                               # (the 1x1 is the downsample: no ReLU)
                Hi, Wi = half(H1, level), half(W1, level)
                Ho, Wo = half(Hi, 1), half(Wi, 1)
                x = torch.randn((m, cin, Hi, Wi), device=dev).abs_().to(dtype)
                w32, stats = weight(cout, cin, k), bn_stats(cout)
                scale, shift = fold(*stats)
                y = core.conv_bn_stride(x, core.conv_pack_weights(w32, dtype), scale, shift, k, 2, relu=relu)
                gy = torch.randn((m, cout, Ho, Wo), device=dev).to(dtype)
                arms = {"new_no_dx": lambda: core.conv_bn_stride_backward(x, w32, scale, y, gy, k, 2, relu=relu,
                                                                          want_features=False)}
                if dx:
                    arms["new"] = lambda: core.conv_bn_stride_backward(x, w32, scale, y, gy, k, 2, relu=relu)
                whole = "new" if dx else "new_no_dx"
                if not a.no_torch:
                    graphs = {}
                    for arm, cl in (("torch_contiguous", False), ("torch_channels_last", True)):
                        xt, wt = x.clone(), w32.to(dtype)
                        if cl:
                            xt, wt = channels_last(xt, wt)
                        xt, wt = xt.requires_grad_(dx), wt.requires_grad_(True)
                        mean, var, gamma, beta = [t.to(dtype) for t in stats]
                        gamma, beta = gamma.requires_grad_(True), beta.requires_grad_(True)
                        yt = F.batch_norm(F.conv2d(xt, wt, stride=2, padding=k // 2), mean, var, gamma, beta, False, 0.0, eps)
                        yt = F.relu(yt) if relu else yt
                        wrt = ((xt,) if dx else ()) + (wt, gamma, beta)
                        graphs[arm] = (yt, wrt, channels_last(gy)[0] if cl else gy)
                        arms[arm] = lambda arm=arm: torch.autograd.grad(graphs[arm][0], graphs[arm][1], graphs[arm][2],
                                                                        retain_graph=True)
                row, med = measure("%s backward_stride %s" % (name, label), arms)
                gb = m * 2 * (cin * Hi * Wi * (2 if dx else 1) + (2 if relu else 1) * cout * Ho * Wo) / 1e9
                tflop = (2 if dx else 1) * 2.0 * k * k * cin * cout * m * Ho * Wo / 1e12
                row.update(shape=[m, cin, cout, Hi, Wi, k, 2], band=core.CONV_BACKWARD_STRIDE_BAND, tflop=round(tflop, 4),
                           compulsory_gb=round(gb, 3), hbm_floor_ms=round(gb / a.hbm_gbs * 1e3, 3),
                           new_share_of_hbm_floor=round(gb / a.hbm_gbs * 1e3 / med[whole], 3),
                           scratch_mb=round(core.conv_bn_stride_backward_scratch_bytes(
                               m, cin, cout, Hi, Wi, k, 2, core.HEAD_F16 if dtype == torch.float16 else core.HEAD_BF16) / 2 ** 20, 1))
                against_torch(row, med, new=whole)
                out["%s_backward_stride_%s" % (name, label)] = row
                note(name, "backward_stride", json.dumps(row))
                del x, y, gy, arms
                if not a.no_torch:
                    del graphs
                torch.cuda.empty_cache()
        if "strided" in parts:
            m, H1, W1 = a.strided_n or n, a.rows, a.cols
            half = lambda v, times: -(-v // 2 ** times)                      # ceil(v / 2^times)
            # (label, channels_in, channels_out, kernel, stride, input rows and cols, residual, relu)
            launches = [("3x3s2_16_32", 16, 32, 3, 2, 0, False, True), ("3x3s2_32_64", 32, 64, 3, 2, 1, False, True),
                        ("3x3s2_64_128", 64, 128, 3, 2, 2, False, True), ("1x1s2_32_64", 32, 64, 1, 2, 1, False, False),
                        ("1x1s2_64_128", 64, 128, 1, 2, 2, False, False), ("3x3s1_res_64", 64, 64, 3, 1, 2, True, True),
                        ("3x3s1_res_128", 128, 128, 3, 1, 3, True, True)]
            for label, cin, cout, k, stride, level, with_res, relu in launches:
                Hi, Wi = half(H1, level), half(W1, level)
                Ho, Wo = -(-Hi // stride), -(-Wi // stride)
                x = torch.randn((m, cin, Hi, Wi), device=dev).abs_().to(dtype)
                res = torch.randn((m, cout, Ho, Wo), device=dev).to(dtype) if with_res else None
                w32, stats = weight(cout, cin, k), bn_stats(cout)
                packed, (scale, shift) = core.conv_pack_weights(w32, dtype), fold(*stats)
                arms = {"new": lambda: core.conv_bn_stride(x, packed, scale, shift, k, stride, residual=res, relu=relu)}
                if not a.no_torch:
                    wd, bn = w32.to(dtype), [t.to(dtype) for t in stats]
                    x_cl, w_cl = channels_last(x, wd)
                    res_cl = channels_last(res)[0] if with_res else None
                    arms["torch_contiguous"] = lambda: torch_conv_bn(x, wd, 1, bn, relu, stride, res)
                    arms["torch_channels_last"] = lambda: torch_conv_bn(x_cl, w_cl, 1, bn, relu, stride, res_cl)
                row, med = measure("%s %s" % (name, label), arms)
                gb = m * 2 * (cin * Hi * Wi + (2 if with_res else 1) * cout * Ho * Wo) / 1e9
                tflop = 2.0 * k * k * cin * cout * m * Ho * Wo / 1e12
                row.update(frames=m, shape_in=[m, cin, Hi, Wi], shape_out=[m, cout, Ho, Wo], compulsory_gb=round(gb, 3),
                           tflop=round(tflop, 4), new_gb_per_s=round(gb / (med["new"] * 1e-3), 1),
                           new_tflops=round(tflop / (med["new"] * 1e-3), 1))
                against_torch(row, med)
                out["%s_%s" % (name, label)] = row
                note(name, label, json.dumps(row))
                del x, res, packed, arms
                if not a.no_torch:
                    del x_cl, res_cl
                torch.cuda.empty_cache()
            layer2 = torch.nn.Sequential(torch.nn.Conv2d(16, 32, 3, stride=2, padding=1, bias=False),
                                         torch.nn.BatchNorm2d(32), torch.nn.ReLU())
            with torch.no_grad():
                mean, var, gamma, beta = (t.cpu() for t in bn_stats(32))
                layer2[0].weight.copy_(weight(32, 16, 3))
                layer2[1].running_mean.copy_(mean), layer2[1].running_var.copy_(var)
                layer2[1].weight.copy_(gamma), layer2[1].bias.copy_(beta)
            layer2.eval()
            blocks = [TorchBlock(32, 64, 1, dtype, stride=2), TorchBlock(64, 64, 1, dtype),
                      TorchBlock(64, 128, 1, dtype, stride=2), TorchBlock(128, 128, 1, dtype)]
            ours = [cnn.StridedConvBnRelu(layer2[0], layer2[1], dtype=dtype)] + \
                   [cnn.StridedResidualBlock(b.to(dev), dtype=dtype) for b in blocks]
            x = torch.randn((m, 16, H1, W1), device=dev).abs_().to(dtype)

            def new():
                y = x
                for layer in ours:
                    y = layer(y)
                return y
            arms = {"new": new}
            if not a.no_torch:
                seq = torch.nn.Sequential(layer2, *blocks).to(device=dev, dtype=dtype).eval()
                seq_cl = copy.deepcopy(seq).to(memory_format=torch.channels_last).eval()
                x_cl, = channels_last(x)
                arms["torch_contiguous"] = lambda: seq(x)
                arms["torch_channels_last"] = lambda: seq_cl(x_cl)
            with torch.no_grad():
                row, med = measure(name + " layer2+layer3+layer4", arms)
            convs = [(layer2[0], 1)] + [(c, lv) for b, lv in zip(blocks, (2, 2, 3, 3)) for c in
                                        [b.conv1, b.conv2] + ([b.downsample[0]] if b.downsample is not None else [])]
            tflop = sum(2.0 * c.weight.numel() * m * half(H1, lv) * half(W1, lv) for c, lv in convs) / 1e12
            row.update(frames=m, shape_in=[m, 16, H1, W1], launches=len(convs), tflop=round(tflop, 3),
                       mfma_floor_ms=round(floor_ms(tflop), 3), new_tflops=round(tflop / (med["new"] * 1e-3), 1))
            against_torch(row, med)
            out[name + "_strided_layers"] = row
            note(name, "strided layers", json.dumps(row))
            del x, ours, arms
            torch.cuda.empty_cache()
        if "stem" in parts:
            m, H1, W1 = a.stem_n or n, a.rows, a.cols
            mean, std = (0.290101, 0.328081, 0.286964), (0.182954, 0.186566, 0.184475)
            image = torch.randint(0, 256, (m, H1, W1, 3), device=dev, dtype=torch.uint8)
            w0, w1, stats0, stats1 = weight(16, 3, 7), weight(16, 16, 3), bn_stats(16), bn_stats(16)
            lut = cnn.input_table(mean, std, dtype).to(dev)
            packed, folds = core.stem_pack_weights(w0, w1, dtype), fold(*stats0) + fold(*stats1)
            arms = {"new": lambda: core.stem(image, lut, packed, *folds),
                    "new_with_mid": lambda: core.stem(image, lut, packed, *folds, want_mid=True)}
            if not a.no_torch:
                w0d, w1d, bn0, bn1 = w0.to(dtype), w1.to(dtype), [t.to(dtype) for t in stats0], [t.to(dtype) for t in stats1]
                w0_cl, w1_cl = channels_last(w0d, w1d)
                mean_t, std_t = (torch.tensor(v, device=dev).view(1, 3, 1, 1) for v in (mean, std))

                def torch_stem(cl):
                    x = ((image.permute(0, 3, 1, 2).float() / 255 - mean_t) / std_t).to(dtype)
                    x = x.contiguous(memory_format=torch.channels_last) if cl else x.contiguous()
                    y = torch_conv_bn(x, w0_cl if cl else w0d, 1, bn0, True)
                    return torch_conv_bn(y, w1_cl if cl else w1d, 1, bn1, True)
                arms["torch_contiguous"] = lambda: torch_stem(False)
                arms["torch_channels_last"] = lambda: torch_stem(True)
            row, med = measure(name + " stem", arms)
            pixels = m * H1 * W1
            gb, tflop = pixels * 35 / 1e9, 2.0 * 16 * (147 + 144) * pixels / 1e12
            row.update(frames=m, shape_in=[m, H1, W1, 3], shape_out=[m, 16, H1, W1], compulsory_gb=round(gb, 3),
                       tflop=round(tflop, 4), new_gb_per_s=round(gb / (med["new"] * 1e-3), 1),
                       new_tflops=round(tflop / (med["new"] * 1e-3), 1),
                       with_mid_gb_per_s=round(pixels * 67 / 1e9 / (med["new_with_mid"] * 1e-3), 1))
            against_torch(row, med)
            out[name + "_stem"] = row
            note(name, "stem", json.dumps(row))
            del image, arms
            torch.cuda.empty_cache()
        if "stem_backward" in parts:
            m, H1, W1, cn = a.stem_n or n, a.rows, a.cols, 32
            mean, std = (0.290101, 0.328081, 0.286964), (0.182954, 0.186566, 0.184475)
            image = torch.randint(0, 256, (m, H1, W1, 3), device=dev, dtype=torch.uint8)
            w0, w1, w2 = weight(16, 3, 7), weight(16, 16, 3), weight(cn, 16, 3)
            stats0, stats1, stats2 = bn_stats(16), bn_stats(16), bn_stats(cn)
            lut = cnn.input_table(mean, std, dtype).to(dev)
            folds = fold(*stats0) + fold(*stats1)
            scale2 = fold(*stats2)[0]
            y, mid = core.stem(image, lut, core.stem_pack_weights(w0, w1, dtype), *folds, want_mid=True)
            gy = torch.randn((m, 16, H1, W1), device=dev).to(dtype)
            Ho, Wo = (H1 + 1) // 2, (W1 + 1) // 2
            gnext = (torch.randn((m, cn, Ho, Wo), device=dev) * (torch.rand((m, cn, Ho, Wo), device=dev) > 0.5)).to(dtype)
            call = lambda **src: core.stem_backward(image, lut, w0, w1, folds[0], folds[2], mid, y, **src)
            arms = {"new": lambda: call(grad_out=gy),
                    "new_next": lambda: call(grad_next=gnext, weight_next=w2, scale_next=scale2)}
            if not a.no_torch:
                graphs = {}
                mean_t, std_t = (torch.tensor(v, device=dev).view(1, 3, 1, 1) for v in (mean, std))
                x = ((image.permute(0, 3, 1, 2).float() / 255 - mean_t) / std_t).to(dtype)
                for arm, cl in (("torch_contiguous", False), ("torch_channels_last", True)):
                    xt, ws = x.clone(), [w0.to(dtype), w1.to(dtype), w2.to(dtype)]
                    if cl:
                        xt, ws = channels_last(xt)[0], channels_last(*ws)
                    ws = [w.requires_grad_(True) for w in ws]
                    bns = [[t.to(dtype) for t in st] for st in (stats0, stats1, stats2)]
                    for bn in bns[:2]:
                        bn[2].requires_grad_(True), bn[3].requires_grad_(True)
                    y1 = torch_conv_bn(torch_conv_bn(xt, ws[0], 1, bns[0], True), ws[1], 1, bns[1], True)
                    y2 = torch_conv_bn(y1, ws[2], 1, bns[2], False, stride=2)         # gnext is already masked
                    wrt = (ws[0], bns[0][2], bns[0][3], ws[1], bns[1][2], bns[1][3])
                    graphs[arm] = (y1, y2, wrt, channels_last(gy)[0] if cl else gy, channels_last(gnext)[0] if cl else gnext)
                    arms[arm] = lambda arm=arm: torch.autograd.grad(graphs[arm][0], graphs[arm][2], graphs[arm][3],
                                                                    retain_graph=True)
                    arms[arm + "_next"] = lambda arm=arm: torch.autograd.grad(graphs[arm][1], graphs[arm][2], graphs[arm][4],
                                                                              retain_graph=True)
            row, med = measure(name + " stem_backward", arms)
            pixels = m * H1 * W1
            # the compulsory bytes once each: the image, dY (or layer2's masked gradient), out and mid
            gb, gb_next = pixels * (3 + 32 + 32 + 32) / 1e9, (pixels * (3 + 32 + 32) + m * cn * Ho * Wo * 2) / 1e9
            row.update(frames=m, shape_in=[m, H1, W1, 3], band=core.STEM_BACKWARD_BAND, segment=core.STEM_BACKWARD_SEGMENT,
                       compulsory_gb=round(gb, 3), hbm_floor_ms=round(gb / a.hbm_gbs * 1e3, 3),
                       new_share_of_hbm_floor=round(gb / a.hbm_gbs * 1e3 / med["new"], 3),
                       next_compulsory_gb=round(gb_next, 3), next_hbm_floor_ms=round(gb_next / a.hbm_gbs * 1e3, 3),
                       next_share_of_hbm_floor=round(gb_next / a.hbm_gbs * 1e3 / med["new_next"], 3),
                       scratch_mb=round(core.stem_backward_scratch_bytes(
                           m, H1, W1, 0, core.HEAD_F16 if dtype == torch.float16 else core.HEAD_BF16) / 2 ** 20, 1))
            against_torch(row, med)
            if not a.no_torch:
                best = min(med["torch_contiguous_next"], med["torch_channels_last_next"])
                row.update(next_torch_best_ms=round(best, 3), next_over_torch_best=round(med["new_next"] / best, 3),
                           next_faster=bool(med["new_next"] < best))
            out[name + "_stem_backward"] = row
            note(name, "stem_backward", json.dumps(row))
            del image, arms, y, mid, gy, gnext
            if not a.no_torch:
                del graphs
            torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
