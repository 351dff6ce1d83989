"""The reference's two "SL" regression losses (tools/CNN_training/losses.py: OffsetLossSL, DisparityOffsetLossSL) on
the device: one call of is_offset_loss per batch (core.offset_loss, include/instance_stixels_core.h f12) gives the
loss, its four parts and the gradient with respect to the prediction, in place of the reference's Python loop per
frame and per instance id and of the autograd replay behind it.

The classes keep the reference's constructor keywords and call signatures.  The weights reach the device as float32
(1e-3 becomes 0.001000000047..), the one deviation from the reference's Python floats.  Predictions in fp16 / bf16 are
converted with .float().

SegmentationHead and SemanticNLLLoss (f14) close the path to the parameters: the head module runs f13's launch in its
forward and one call of is_segmentation_head_backward in its backward, so a model is trained with the numerics it is
deployed with, and a training step gives the same bytes on every run.  SemanticNLLLossUp (f16) is the loss of the
full-resolution models: the same head, scored through the reference's fixed bilinear `up` layer."""
import math

import torch

from . import core


class _OffsetLossFunction(torch.autograd.Function):
    """The forward makes the gradient at unit scale and keeps it; the backward multiplies it by grad_output on the
    device, so nothing is computed twice."""

    @staticmethod
    def forward(ctx, prediction, ids8, disparity8_u16, weights, abs_variance, capacity, check):
        loss5, terms, grad = core.offset_loss(prediction.detach(), ids8, disparity8_u16, weights=weights,
                                              abs_variance=abs_variance, capacity=capacity, check=check)
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(terms)
        return loss5, terms

    @staticmethod
    def backward(ctx, grad_loss5, grad_terms):
        grad, = ctx.saved_tensors
        # only the loss itself (element 0) is differentiable; the four sums are reports
        return grad * grad_loss5[0], None, None, None, None, None, None


def _squeeze_channel(t):
    """[n][1][H][W] -> [n][H][W]; anything else as it is."""
    return t[:, 0] if t.dim() == 4 and t.shape[1] == 1 else t


def _class_planes(output, n_classes):
    """The head's output as float32, its first n_classes channels where that is given (a slice, read in place)."""
    out = output if output.dtype == torch.float32 else output.float()
    return out if n_classes is None else out[:, :int(n_classes)]


def _ids8(batch_instance_gt, device):
    ids = _squeeze_channel(batch_instance_gt)
    if ids.dim() != 3:
        raise core.CoreError("the instance ids must be [n][Hs][Ws] or [n][1][Hs][Ws]")
    return ids.to(device=device, dtype=torch.int32).contiguous()


def _disparity8(batch_disparity_gt, device):
    """uint16 raw as it is; anything else is the reference's tensor of integral q = raw // 256 in 0 .. 255."""
    d = _squeeze_channel(batch_disparity_gt)
    if d.dim() != 3:
        raise core.CoreError("the disparity must be [n][Hs][Ws] or [n][1][Hs][Ws]")
    d = d.to(device)
    if d.dtype == torch.uint16:
        return d.contiguous()
    return (d.to(torch.int32) << 8).to(torch.uint16).contiguous()


def _prediction(batch_prediction, planes):
    p = batch_prediction
    if not p.is_cuda or p.dim() != 4 or p.shape[1] != planes:
        raise core.CoreError(f"the prediction must be a device tensor [n][{planes}][Hs][Ws]")
    return p if p.dtype == torch.float32 else p.float()


class DisparityOffsetLossSL:
    """losses.py:24-125.  batch_prediction [n][3][Hs][Ws] (disp, off_y, off_x), batch_instance_gt the instance ids
    mode-downsampled by 8, batch_disparity_gt the disparity mode-downsampled by 8 as integral q = raw // 256 (the
    reference's tensor) or as raw uint16.  Returns the loss (loss.backward() works), with separate=True the five
    values (loss, offset_mean, offset_variance, disparity_mean, disparity_variance) as one detached tensor on the
    device.  capacity / check: see core.offset_loss."""

    def __init__(self, offset_mean_weight=1e-3, offset_variance_weight=1e-4, disparity_mean_weight=1e-3,
                 disparity_variance_weight=1e-4, abs_variance=False, capacity=0, check=True):
        self.weights = {"offset_mean": offset_mean_weight, "offset_variance": offset_variance_weight,
                        "disparity_mean": disparity_mean_weight, "disparity_variance": disparity_variance_weight}
        self.abs_variance = abs_variance
        self.capacity, self.check = capacity, check

    def __call__(self, batch_prediction, batch_instance_gt, batch_disparity_gt, separate=False):
        p = _prediction(batch_prediction, 3)
        w = tuple(self.weights[k] for k in ("offset_mean", "offset_variance", "disparity_mean", "disparity_variance"))
        loss5, _ = _OffsetLossFunction.apply(p, _ids8(batch_instance_gt, p.device),
                                             _disparity8(batch_disparity_gt, p.device), w, bool(self.abs_variance),
                                             self.capacity, self.check)
        return loss5.detach() if separate else loss5[0]


class OffsetLossSL:
    """losses.py:127-175.  batch_prediction [n][2][Hs][Ws] (off_y, off_x).  As the reference's, it has the variance
    in its population form only: further keywords (abs_variance among them) are accepted and ignored."""

    def __init__(self, offset_mean_weight=1e-3, offset_variance_weight=1e-4, capacity=0, check=True, **kwargs):
        self.mean_weight = offset_mean_weight
        self.variance_weight = offset_variance_weight
        self.capacity, self.check = capacity, check

    def __call__(self, batch_prediction, batch_instance_gt):
        p = _prediction(batch_prediction, 2)
        w = (self.mean_weight, self.variance_weight, 0.0, 0.0)
        loss5, _ = _OffsetLossFunction.apply(p, _ids8(batch_instance_gt, p.device), None, w, False, self.capacity,
                                             self.check)
        return loss5[0]


class _SegmentationHeadFunction(torch.autograd.Function):
    """Forward: f13's launch (the float output only).  Backward: one call of is_segmentation_head_backward that asks
    for the gradients autograd needs and no others."""

    @staticmethod
    def forward(ctx, features, weight, bias, n_classes):
        rows8 = features.shape[2]
        p2s = 1 << rows8.bit_length()                     # a power of two >= rows8 + 1; the int tensor is not made
        y = core.segmentation_head(features.detach(), weight.detach(), bias.detach(), n_classes, p2s,
                                   want_segmentation=False)
        ctx.save_for_backward(features, weight, y)
        ctx.n_classes = n_classes
        return y

    @staticmethod
    def backward(ctx, grad_y):
        features, weight, y = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        if not (need_x or need_w or need_b):
            return None, None, None, None
        g = core.segmentation_head_backward(features, weight, y, grad_y.float(), ctx.n_classes, want_features=need_x,
                                            want_weight=need_w, want_bias=need_b)
        gw = g["weight"].view(weight.shape) if need_w else None
        return g.get("features"), gw, g.get("bias"), None


class SegmentationHead(torch.nn.Module):
    """The head of the reference's models (DRNDownsampled.py:80-102, 119-137) on the device with fixed numerics: the
    1x1 convolution `seg`, -log_softmax over the first n_classes channels, the regression channels behind them.
    `weight` [channels][K][1][1] and `bias` [channels] take the reference's `seg` state; the initialisation is the
    reference's (DRNDownsampled.py:82-85).  forward(features) returns float32 [n][channels][rows8][cols8], features
    being float32, float16 or bfloat16 [n][K][rows8][cols8] on the device; it is differentiable in the features, the
    weight and the bias.  clamp = (channel, lo, hi) clamps one regression channel in eval mode only, as
    DRNDSOffsetDisparity does (:133-134); that output cannot be differentiated."""

    def __init__(self, in_features, n_classes, n_regression=2, clamp=None):
        super().__init__()
        channels = n_classes + n_regression
        if not 1 <= n_classes <= channels <= core.HEAD_MAX_CHANNELS:
            raise core.CoreError(f"n_classes >= 1, n_regression >= 0 and at most {core.HEAD_MAX_CHANNELS} channels")
        self.n_classes, self.clamp = int(n_classes), clamp
        self.weight = torch.nn.Parameter(torch.empty(channels, in_features, 1, 1))
        self.bias = torch.nn.Parameter(torch.zeros(channels))
        with torch.no_grad():
            self.weight.normal_(0, math.sqrt(2.0 / channels))   # n = 1 * 1 * out_channels

    def forward(self, features):
        if not self.training and self.clamp is not None:
            if torch.is_grad_enabled() and (features.requires_grad or self.weight.requires_grad
                                            or self.bias.requires_grad):
                raise core.CoreError("the clamped eval-mode output is not differentiable: call it under "
                                     "torch.no_grad(), or train() the module")
            p2s = 1 << int(features.shape[2]).bit_length()
            return core.segmentation_head(features, self.weight, self.bias, self.n_classes, p2s,
                                          want_segmentation=False, clamp=self.clamp)
        return _SegmentationHeadFunction.apply(features, self.weight, self.bias, self.n_classes)


class _SemanticNLLFunction(torch.autograd.Function):
    """As _OffsetLossFunction: the forward makes the gradient at unit scale, the backward scales it.  loss_name:
    "semantic_nll", or "semantic_nll_up" for the loss through the fixed `up` layer (f16), looked up in core per call."""

    @staticmethod
    def forward(ctx, classes, target, ignore_index, check, loss_name):
        loss, _, _, grad = getattr(core, loss_name)(classes.detach(), target, classes.shape[1],
                                                    ignore_index=ignore_index, grad=True, check=check)
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        grad, = ctx.saved_tensors
        return grad * grad_loss[0], None, None, None, None


class SemanticNLLLoss:
    """nn.NLLLoss(reduction='mean', ignore_index=255) of the reference's training (train.py:281-282, 325-326) on the
    head's class channels, which hold -log p: output [n][C][rows8][cols8] float32, all of whose channels are classes
    unless n_classes says that only the first n_classes are (a channel slice of the head's output is read in place);
    target [n][rows8][cols8] uint8 or int32 (other integer types are converted to int32).  Returns the loss, a scalar
    on the device; loss.backward() works.  check: see core.semantic_nll."""

    def __init__(self, ignore_index=255, n_classes=None, check=True):
        self.ignore_index, self.n_classes, self.check = int(ignore_index), n_classes, check

    def __call__(self, output, target):
        t = _squeeze_channel(target).to(output.device)
        if t.dtype not in (torch.uint8, torch.int32):
            t = t.to(torch.int32)
        out = _class_planes(output, self.n_classes)
        return _SemanticNLLFunction.apply(out, t, self.ignore_index, self.check, "semantic_nll")[0]


class SemanticNLLLossUp:
    """The classification loss of the reference's full-resolution models (DRNSeg.py:46-225: seg -> up -> LogSoftmax;
    train.py:69-232: nn.NLLLoss(reduction='mean', ignore_index=255) on full-resolution ground truth) on the head's
    1/8-resolution output, whose class channels hold -log p: output [n][C][rows8][cols8] float32, all of whose channels
    are classes unless n_classes says that only the first n_classes are (a channel slice is read in place);
    target_full [n][8 * rows8][cols >= 8 * cols8] or [n][1][..][..] of class ids, converted to uint8 after a range
    check (one synchronisation, for other integer types only).  The upsampled planes are never stored.  Returns the
    loss, a scalar on the device; loss.backward() works.  check: see core.semantic_nll_up."""

    def __init__(self, ignore_index=255, n_classes=None, check=True):
        self.ignore_index, self.n_classes, self.check = int(ignore_index), n_classes, check

    def __call__(self, output, target_full):
        t = _squeeze_channel(target_full).to(output.device)
        if t.dtype != torch.uint8:
            if t.is_floating_point() or t.dtype == torch.bool:
                raise core.CoreError("target_full must hold integer class ids")
            if t.numel() and (int(t.min()) < 0 or int(t.max()) > 255):
                raise core.CoreError("target_full holds class ids outside [0, 255]")
            t = t.to(torch.uint8)
        out = _class_planes(output, self.n_classes)
        return _SemanticNLLFunction.apply(out, t, self.ignore_index, self.check, "semantic_nll_up")[0]
