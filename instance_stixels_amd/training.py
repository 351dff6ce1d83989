"""The reference's two "SL" regression losses (tools/CNN_training/losses.py: OffsetLossSL, DisparityOffsetLossSL) on
the device: one call of is_offset_loss per batch (core.offset_loss, include/instance_stixels_core.h f12) gives the
loss, its four parts and the gradient with respect to the prediction, in place of the reference's Python loop per
frame and per instance id and of the autograd replay behind it.

The classes keep the reference's constructor keywords and call signatures.  The weights reach the device as float32
(1e-3 becomes 0.001000000047..), the one deviation from the reference's Python floats.  Predictions in fp16 / bf16 are
converted with .float()."""
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


def _ids8(batch_instance_gt, device):
    ids = batch_instance_gt
    if ids.dim() == 4 and ids.shape[1] == 1:
        ids = ids[:, 0]
    if ids.dim() != 3:
        raise core.CoreError("the instance ids must be [n][Hs][Ws] or [n][1][Hs][Ws]")
    return ids.to(device=device, dtype=torch.int32).contiguous()


def _disparity8(batch_disparity_gt, device):
    """uint16 raw as it is; anything else is the reference's tensor of integral q = raw // 256 in 0 .. 255."""
    d = batch_disparity_gt
    if d.dim() == 4 and d.shape[1] == 1:
        d = d[:, 0]
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
