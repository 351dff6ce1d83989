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


# ---- f21: conv + frozen BatchNorm (+ residual) (+ ReLU) with a backward pass on the device ----

def _frozen_bn(bn, name):
    """The checks of a BatchNorm2d whose running statistics the modules below freeze."""
    if not isinstance(bn, torch.nn.BatchNorm2d):
        raise core.CoreError(f"{name} must be a BatchNorm2d, not {type(bn).__name__}")
    if bn.training:
        raise core.CoreError(f"{name} is in training mode: batch statistics are another forward and are not built; "
                             "put it into eval() to freeze it at its running statistics")
    if bn.running_mean is None or bn.running_var is None:
        raise core.CoreError(f"{name} tracks no running statistics")


class _FrozenBatchNorm(torch.nn.Module):
    """The affine pair of a BatchNorm2d as Parameters, its running statistics as buffers that are never updated.
    fold() is cnn.fold_batchnorm's (scale, shift), value for value -- float64, rounded once each -- made of
    differentiable torch ops on the parameters' device, so autograd reaches weight and bias by itself."""

    def __init__(self, bn):
        super().__init__()
        n = bn.num_features
        self.weight = torch.nn.Parameter(bn.weight.detach().clone().float() if bn.weight is not None else torch.ones(n))
        self.bias = torch.nn.Parameter(bn.bias.detach().clone().float() if bn.bias is not None else torch.zeros(n))
        self.register_buffer("running_mean", bn.running_mean.detach().clone().float())
        self.register_buffer("running_var", bn.running_var.detach().clone().float())
        self.eps = float(bn.eps)

    def fold(self):
        scale = self.weight.double() / torch.sqrt(self.running_var.double() + self.eps)
        shift = self.bias.double() - self.running_mean.double() * scale
        return scale.float(), shift.float()


def _half_features(x):
    if not torch.is_tensor(x) or not x.is_cuda or x.dim() != 4 or x.dtype not in (torch.float16, torch.bfloat16):
        raise core.CoreError("the features must be a float16 or bfloat16 device tensor [n][channels][rows8][cols8] "
                             "(fp32 features are not built: convert them first)")


def _conv(x, packed, scale, shift, kernel, stride, dilation, **more):
    """core.conv_bn at stride 1 (f21's modules keep their call), core.conv_bn_stride at stride 2."""
    if stride == 1:
        return core.conv_bn(x, packed, scale, shift, kernel, dilation, **more)
    return core.conv_bn_stride(x, packed, scale, shift, kernel, stride, dilation, **more)


def _conv_backward(x, weight, scale, out, grad_out, kernel, stride, dilation, **more):
    """core.conv_bn_backward at stride 1, core.conv_bn_stride_backward at stride 2."""
    if stride == 1:
        return core.conv_bn_backward(x, weight, scale, out, grad_out, kernel, dilation, **more)
    return core.conv_bn_stride_backward(x, weight, scale, out, grad_out, kernel, stride, dilation, **more)


class _ConvBnFunction(torch.autograd.Function):
    """Forward: the pack of the current weight and one launch of core.conv_bn (stride 2: core.conv_bn_stride).
    Backward: one call of core.conv_bn_backward (core.conv_bn_stride_backward) that asks for the gradients autograd
    needs and no others."""

    @staticmethod
    def forward(ctx, x, weight, scale, shift, kernel, dilation, relu, stride=1):
        packed = core.conv_pack_weights(weight.detach(), x.dtype)
        out = _conv(x.detach(), packed, scale.detach(), shift.detach(), kernel, stride, dilation, relu=relu)
        ctx.save_for_backward(x, weight, scale, out)
        ctx.conv = (kernel, dilation, relu, stride)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, weight, scale, out = ctx.saved_tensors
        kernel, dilation, relu, stride = ctx.conv
        need = ctx.needs_input_grad[:4]
        if not any(need):
            return (None,) * 8
        g = _conv_backward(x, weight, scale, out, grad_out, kernel, stride, dilation, relu=relu, want_features=need[0],
                           want_weight=need[1], want_scale=need[2], want_shift=need[3])
        return g.get("features"), g.get("weight"), g.get("scale"), g.get("shift"), None, None, None, None


class ConvBnReLU(torch.nn.Module):
    """Conv2d(3x3, padding = dilation, stride 1, bias=False) + BatchNorm2d frozen at its running statistics + ReLU, as
    cnn.ConvBnRelu checks the pair, trainable: `weight` is the fp32 master weight, bn.weight and bn.bias the affine
    pair; the running statistics are buffers that no forward updates, whatever train() says.  forward(features) runs
    is_conv_bn on features of float16 or bfloat16 and returns their dtype; its backward is one call of
    is_conv_bn_backward (instance_stixels_core.h f21).  Batch-statistics BatchNorm, stride 2 and fp32 features raise
    CoreError before anything is packed."""

    strides = (1,)     # the strides of conv that the class accepts

    def __init__(self, conv, bn, relu=True):
        super().__init__()
        from . import cnn
        self.dilation = cnn._dilated3x3(conv, "conv", self.strides)
        self.stride = int(conv.stride[0])
        _frozen_bn(bn, "bn")
        if bn.num_features != conv.out_channels:
            raise core.CoreError(f"bn has {bn.num_features} channels, conv {conv.out_channels}")
        self.kernel, self.relu = 3, bool(relu)
        self.weight = torch.nn.Parameter(conv.weight.detach().clone().float())
        self.bn = _FrozenBatchNorm(bn)

    def forward(self, features):
        _half_features(features)
        scale, shift = self.bn.fold()
        return _ConvBnFunction.apply(features, self.weight, scale, shift, self.kernel, self.dilation, self.relu,
                                     self.stride)


class StridedConvBnReLU(ConvBnReLU):
    """ConvBnReLU for a conv of stride 1 or 2, as cnn.StridedConvBnRelu checks the pair (layer2 of the reference: stride
    2, padding 1, dilation 1).  Its forward is cnn.StridedConvBnRelu's launch and bytes; its backward at stride 2 is
    one call of is_conv_bn_stride_backward (instance_stixels_core.h f22).  The gradient of the features needs
    channels_in % 32 == 0: layer2 itself (16 channels in) trains its weight and BatchNorm pair behind a frozen stem."""

    strides = (1, 2)


def _basic_block_layout(block, strides=(1,)):
    """The checks of a BasicBlock-shaped `block` (conv1, bn1, conv2, bn2, downsample, residual), cnn.ResidualBlock's
    (strides (1, 2): cnn.StridedResidualBlock's), made before anything is folded or packed: (conv1's dilation, conv2's
    dilation, whether the block adds a residual, the downsample's (Conv2d, BatchNorm2d) or None).  conv1's stride, and
    with it the downsample's, is out of `strides`."""
    from . import cnn
    if hasattr(block, "conv3"):
        raise core.CoreError("a block with conv3 is a Bottleneck: only BasicBlock is covered")
    d1, d2 = cnn._dilated3x3(block.conv1, "conv1", strides), cnn._dilated3x3(block.conv2, "conv2")
    stride = int(block.conv1.stride[0])
    c_in, c_mid, c_out = block.conv1.in_channels, block.conv1.out_channels, block.conv2.out_channels
    if block.conv2.in_channels != c_mid or block.bn1.num_features != c_mid or block.bn2.num_features != c_out:
        raise core.CoreError("conv1, bn1, conv2 and bn2 disagree on their channels")
    residual = bool(block.residual)
    down = block.downsample if residual else None      # (the reference computes and drops it otherwise)
    if down is None:
        if residual and stride != 1:
            raise core.CoreError(f"conv1 has stride {stride} and the block no downsample: the input cannot be the residual")
        if residual and c_in != c_out:
            raise core.CoreError(f"residual=True without a downsample needs equal channels, not {c_in} -> {c_out}")
        return d1, d2, residual, None
    mods = list(down) if isinstance(down, torch.nn.Sequential) else []
    if len(mods) != 2 or not isinstance(mods[0], torch.nn.Conv2d) or not isinstance(mods[1], torch.nn.BatchNorm2d) \
            or tuple(mods[0].kernel_size) != (1, 1) or mods[0].bias is not None or mods[0].groups != 1 \
            or tuple(mods[0].padding) != (0, 0) or mods[0].in_channels != c_in or mods[0].out_channels != c_out \
            or mods[1].num_features != c_out:
        raise core.CoreError("downsample must be nn.Sequential(Conv2d(kernel_size=1, bias=False), BatchNorm2d) "
                             "from the block's input to its output channels")
    if tuple(strides) == (1,) and tuple(mods[0].stride) != (1, 1):
        raise core.CoreError(f"downsample has stride {tuple(mods[0].stride)}: only stride 1 is covered")
    if tuple(mods[0].stride) != (stride, stride):
        raise core.CoreError(f"downsample has stride {tuple(mods[0].stride)}, conv1 {(stride, stride)}: the "
                             "residual must have the shape of conv2's output")
    return d1, d2, residual, (mods[0], mods[1])


class _BasicBlockFunction(torch.autograd.Function):
    """The whole block as one node.  inputs: x, then (weight, scale, shift) of conv1, conv2 and, with a downsample, of
    it.  The backward is conv2's call, the downsample's and conv1's, with nothing of torch's in between: conv2's call
    hands out the masked gradient (want_pre), which is the gradient with respect to the residual operand, and the
    second path into x joins conv1's dX inside its launch (features_add)."""

    @staticmethod
    def forward(ctx, x, d1, d2, residual, *params):
        stride = 1
        if isinstance(params[-1], int):                    # (StridedBasicBlock's: conv1's and the downsample's stride)
            params, stride = params[:-1], params[-1]
        w1, s1, b1, w2, s2, b2 = params[:6]
        down = params[6:] if len(params) == 9 else None
        xd = x.detach()
        pack = lambda w: core.conv_pack_weights(w.detach(), x.dtype)
        y1 = _conv(xd, pack(w1), s1.detach(), b1.detach(), 3, stride, d1, relu=True)
        res = None
        if residual:
            res = _conv(xd, pack(down[0]), down[1].detach(), down[2].detach(), 1, stride, 1, relu=False) if down else xd
        out = core.conv_bn(y1, pack(w2), s2.detach(), b2.detach(), 3, d2, residual=res, relu=True)
        ctx.save_for_backward(x, y1, out, w1, s1, w2, s2, *((down[0], down[1]) if down else ()))
        ctx.block = (d1, d2, residual, down is not None, stride)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, y1, out, w1, s1, w2, s2 = ctx.saved_tensors[:7]
        d1, d2, residual, has_down, stride = ctx.block
        need = ctx.needs_input_grad
        need_x, n1, n2, nd = need[0], need[4:7], need[7:10], need[10:13] if has_down else (False,) * 3
        through1 = need_x or any(n1)                       # anything behind conv1's output
        side = residual and (need_x or any(nd))            # the residual operand's gradient is used
        grads = [None] * (4 + (9 if has_down else 6) + (stride != 1))
        if not (through1 or side or any(n2)):
            return tuple(grads)
        g2 = core.conv_bn_backward(y1, w2, s2, out, grad_out, 3, d2, relu=True, want_features=through1,
                                   want_weight=n2[0], want_scale=n2[1], want_shift=n2[2], want_pre=side)
        grads[7:10] = g2.get("weight"), g2.get("scale"), g2.get("shift")
        add = None
        if side and has_down:
            wd, sd = ctx.saved_tensors[7:9]
            gd = _conv_backward(x, wd, sd, None, g2["pre"], 1, stride, 1, relu=False, want_features=need_x,
                                want_weight=nd[0], want_scale=nd[1], want_shift=nd[2])
            grads[10:13] = gd.get("weight"), gd.get("scale"), gd.get("shift")
            add = gd.get("features")
        elif side:
            add = g2["pre"]                                # x itself was the residual
        if through1:
            g1 = _conv_backward(x, w1, s1, y1, g2["features"], 3, stride, d1, relu=True, want_features=need_x,
                                want_weight=n1[0], want_scale=n1[1], want_shift=n1[2],
                                features_add=add if need_x else None)
            grads[0] = g1.get("features")
            grads[4:7] = g1.get("weight"), g1.get("scale"), g1.get("shift")
        return tuple(grads)


class BasicBlock(torch.nn.Module):
    """One BasicBlock of the reference (drn.py:54-87) with its BatchNorms frozen at their running statistics, as
    cnn.ResidualBlock checks it, trainable: conv1.weight, conv2.weight (and downsample's) are fp32 master weights, the
    BatchNorm affine pairs Parameters.  The forward is cnn.ResidualBlock's launches; the whole block is ONE autograd
    node whose backward is 2 calls of is_conv_bn_backward, 3 with a downsample, and no torch kernel between them.
    Stride 2, batch statistics and fp32 features raise CoreError before anything is packed."""

    strides = (1,)     # the strides of conv1 (and with it of the downsample) that the class accepts; conv2 has 1

    def __init__(self, block):
        super().__init__()
        self.d1, self.d2, self.residual, down = _basic_block_layout(block, self.strides)
        self.stride = int(block.conv1.stride[0])
        for name, bn in (("bn1", block.bn1), ("bn2", block.bn2)) + ((("downsample's bn", down[1]),) if down else ()):
            _frozen_bn(bn, name)
        self.weight1 = torch.nn.Parameter(block.conv1.weight.detach().clone().float())
        self.weight2 = torch.nn.Parameter(block.conv2.weight.detach().clone().float())
        self.bn1, self.bn2 = _FrozenBatchNorm(block.bn1), _FrozenBatchNorm(block.bn2)
        self.weight_down = torch.nn.Parameter(down[0].weight.detach().clone().float()) if down else None
        self.bn_down = _FrozenBatchNorm(down[1]) if down else None

    def forward(self, features):
        _half_features(features)
        params = [self.weight1, *self.bn1.fold(), self.weight2, *self.bn2.fold()]
        if self.weight_down is not None:
            params += [self.weight_down, *self.bn_down.fold()]
        if self.stride != 1:
            params.append(self.stride)
        return _BasicBlockFunction.apply(features, self.d1, self.d2, self.residual, *params)


class StridedBasicBlock(BasicBlock):
    """BasicBlock for a block whose conv1 has stride 1 or 2, as cnn.StridedResidualBlock checks it (the first blocks of
    layer3 and layer4: conv1 3x3 stride 2, downsample 1x1 stride 2 + BatchNorm, conv2 3x3 stride 1).  The forward is
    cnn.StridedResidualBlock's launches and bytes; the block is ONE autograd node whose backward is conv2's call of
    is_conv_bn_backward with the masked gradient handed out, the downsample's call of is_conv_bn_stride_backward and
    conv1's, which takes the downsample's dX as features_add: no torch kernel in between."""

    strides = (1, 2)


class DrnLayers(torch.nn.Module):
    """layer2 -> layer3 -> ... -> layer8 of the reference's base as one trainable chain: layer1's output [n][16][rows]
    [cols] in float16 or bfloat16 in, layer8's output at 1/8 resolution out, which feeds SegmentationHead.  A layer
    that is nn.Sequential(Conv2d, BatchNorm2d, ReLU) (layer2, layer7, layer8) becomes a StridedConvBnReLU, every other
    layer a sequence of StridedBasicBlocks; every BatchNorm is frozen at its running statistics.  The stem is frozen:
    an input that requires grad raises CoreError, because dX at layer2's 16 channels is not built."""

    def __init__(self, layer2, layer3, layer4, layer5, layer6, layer7, layer8):
        super().__init__()
        from . import cnn
        mods = []
        for i, layer in enumerate((layer2, layer3, layer4, layer5, layer6, layer7, layer8)):
            name = f"layer{i + 2}"
            if not isinstance(layer, torch.nn.Sequential):
                raise core.CoreError(f"{name} must be an nn.Sequential, not {type(layer).__name__}")
            if len(layer) and isinstance(layer[0], torch.nn.Conv2d):
                mods.append(StridedConvBnReLU(*cnn._conv_bn_relu_of(layer, name)))
            else:
                mods.extend(StridedBasicBlock(b) for b in layer)
        self.layers = torch.nn.ModuleList(mods)

    def forward(self, features):
        if torch.is_tensor(features) and features.requires_grad:
            raise core.CoreError("the input of DrnLayers requires grad: the stem is frozen, and the gradient of layer2's "
                                 "16-channel input is not built")
        _half_features(features)
        x = features
        for layer in self.layers:
            x = layer(x)
        return x


# ---- f23: the stem with a backward pass on the device ----

class _StemFunction(torch.autograd.Function):
    """Forward: the pack of the current weights and one launch of core.stem with mid kept.  Backward: one call of
    core.stem_backward that asks for the gradients autograd needs and no others."""

    @staticmethod
    def forward(ctx, image, lut, w0, scale0, shift0, w1, scale1, shift1):
        packed = core.stem_pack_weights(w0.detach(), w1.detach(), lut.dtype, device=image.device)
        out, mid = core.stem(image, lut, packed, scale0.detach(), shift0.detach(), scale1.detach(), shift1.detach(),
                             want_mid=True)
        ctx.save_for_backward(image, lut, w0, scale0, w1, scale1, mid, out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        image, lut, w0, scale0, w1, scale1, mid, out = ctx.saved_tensors
        need = ctx.needs_input_grad[2:]
        if not any(need):
            return (None,) * 8
        g = core.stem_backward(image, lut, w0, w1, scale0, scale1, mid, out, grad_out=grad_out, want_weight0=need[0],
                               want_scale0=need[1], want_shift0=need[2], want_weight1=need[3], want_scale1=need[4],
                               want_shift1=need[5])
        return (None, None, g.get("weight0"), g.get("scale0"), g.get("shift0"), g.get("weight1"), g.get("scale1"),
                g.get("shift1"))


class Stem(torch.nn.Module):
    """layer0 and layer1 of the reference's drn_d_22 behind the image's table, as cnn.DrnStem checks them, trainable:
    `weight0` and `weight1` are the fp32 master weights, bn0 and bn1 the affine pairs of the two BatchNorms, frozen at
    their running statistics.  forward(image) takes the uint8 image [n][rows][cols][3] on the device and returns
    layer1's output [n][16][rows][cols] in `dtype`, the bytes of cnn.DrnStem; it is ONE autograd node whose backward is
    one call of is_stem_backward (instance_stixels_core.h f23) on the gradient its consumer gives.  There is no
    gradient for the image or the table.  Everything is checked before anything is packed."""

    def __init__(self, layer0, layer1, mean, std, dtype=torch.bfloat16):
        super().__init__()
        from . import cnn
        conv0, bn0 = cnn._stem_conv(layer0, "layer0", 3, 7, 3, "")
        conv1, bn1 = cnn._stem_conv(layer1, "layer1", 16, 3, 1,
                                    " (layers[0] > 1 repeats the three: only layers[0] == 1 is covered)")
        _frozen_bn(bn0, "layer0's bn")
        _frozen_bn(bn1, "layer1's bn")
        self.dtype = dtype
        self.register_buffer("lut", cnn.input_table(mean, std, dtype))
        self.weight0 = torch.nn.Parameter(conv0.weight.detach().clone().float())
        self.weight1 = torch.nn.Parameter(conv1.weight.detach().clone().float())
        self.bn0, self.bn1 = _FrozenBatchNorm(bn0), _FrozenBatchNorm(bn1)

    def forward(self, image):
        if not torch.is_tensor(image) or not image.is_cuda or image.dtype != torch.uint8 or image.dim() != 4 or \
                int(image.shape[3]) != 3:
            raise core.CoreError("image must be a uint8 device tensor [n][rows][cols][3]")
        scale0, shift0 = self.bn0.fold()
        scale1, shift1 = self.bn1.fold()
        return _StemFunction.apply(image, self.lut, self.weight0, scale0, shift0, self.weight1, scale1, shift1)


class _StemLayer2Function(torch.autograd.Function):
    """The stem and layer2 as ONE autograd node.  Forward: core.stem with mid kept, then layer2's launch of
    core.conv_bn_stride.  Backward: core.conv_bn_stride_backward for layer2's parameters and its masked gradient, then
    one core.stem_backward that takes that masked gradient as its source: the gradient with respect to layer1's output
    is formed inside the library, and no torch kernel runs between the two calls."""

    @staticmethod
    def forward(ctx, image, lut, w0, scale0, shift0, w1, scale1, shift1, w2, scale2, shift2):
        packed = core.stem_pack_weights(w0.detach(), w1.detach(), lut.dtype, device=image.device)
        out1, mid = core.stem(image, lut, packed, scale0.detach(), shift0.detach(), scale1.detach(), shift1.detach(),
                              want_mid=True)
        packed2 = core.conv_pack_weights(w2.detach(), lut.dtype)
        out2 = core.conv_bn_stride(out1, packed2, scale2.detach(), shift2.detach(), 3, 2, 1, relu=True)
        ctx.save_for_backward(image, lut, w0, scale0, w1, scale1, mid, out1, w2, scale2, out2)
        return out2

    @staticmethod
    def backward(ctx, grad_out):
        image, lut, w0, scale0, w1, scale1, mid, out1, w2, scale2, out2 = ctx.saved_tensors
        need = ctx.needs_input_grad[2:]
        if not any(need):
            return (None,) * 11
        stem_needs = any(need[:6])
        g2 = core.conv_bn_stride_backward(out1, w2, scale2, out2, grad_out, 3, 2, want_features=False, want_weight=need[6],
                                          want_scale=need[7], want_shift=need[8], want_pre=stem_needs)
        g = {}
        if stem_needs:
            g = core.stem_backward(image, lut, w0, w1, scale0, scale1, mid, out1, grad_next=g2["pre"], weight_next=w2,
                                   scale_next=scale2, want_weight0=need[0], want_scale0=need[1], want_shift0=need[2],
                                   want_weight1=need[3], want_scale1=need[4], want_shift1=need[5])
        return (None, None, g.get("weight0"), g.get("scale0"), g.get("shift0"), g.get("weight1"), g.get("scale1"),
                g.get("shift1"), g2.get("weight"), g2.get("scale"), g2.get("shift"))


class Drn(torch.nn.Module):
    """The whole base of the reference's drn_d_22, trainable: the uint8 image [n][rows][cols][3] on the device in,
    layer8's output at 1/8 resolution in `dtype` out, which feeds SegmentationHead.  `stem` is a Stem (layer0, layer1)
    and `layers` a DrnLayers (layer2 .. layer8), whose checks and parameters they are; the stem and layer2 run as one
    autograd node (_StemLayer2Function), layer3 .. layer8 are DrnLayers' modules as they are.  Every BatchNorm is
    frozen at its running statistics.  layer2 must be the reference's Conv2d(16, channels, 3, stride 2, padding 1) with
    channels a multiple of 32 in [32, 128]."""

    def __init__(self, layer0, layer1, layer2, layer3, layer4, layer5, layer6, layer7, layer8, mean, std,
                 dtype=torch.bfloat16):
        super().__init__()
        self.stem = Stem(layer0, layer1, mean, std, dtype)
        self.layers = DrnLayers(layer2, layer3, layer4, layer5, layer6, layer7, layer8)
        first = self.layers.layers[0]
        cn = int(first.weight.shape[0]) if isinstance(first, StridedConvBnReLU) else 0
        if cn == 0 or int(first.weight.shape[1]) != 16 or first.stride != 2 or first.dilation != 1 or not first.relu:
            raise core.CoreError("layer2 must be nn.Sequential(Conv2d(16, channels, 3, stride=2, padding=1, bias=False), "
                                 "BatchNorm2d, ReLU)")
        if cn % 32 or not 32 <= cn <= 128:
            raise core.CoreError(f"layer2 has {cn} channels: the stem's backward takes a multiple of 32 in [32, 128]")
        self.dtype = dtype

    @classmethod
    def from_base(cls, base, mean, std, dtype=torch.bfloat16):
        """base: the reference's model.base, the nn.Sequential of the nine children layer0 .. layer8."""
        layers = list(base)
        if len(layers) != 9:
            raise core.CoreError(f"base has {len(layers)} children, not the nine layer0 .. layer8")
        return cls(*layers, mean, std, dtype=dtype)

    def forward(self, image):
        if not torch.is_tensor(image) or not image.is_cuda or image.dtype != torch.uint8 or image.dim() != 4 or \
                int(image.shape[3]) != 3:
            raise core.CoreError("image must be a uint8 device tensor [n][rows][cols][3]")
        stem, first = self.stem, self.layers.layers[0]
        x = _StemLayer2Function.apply(image, stem.lut, stem.weight0, *stem.bn0.fold(), stem.weight1, *stem.bn1.fold(),
                                      first.weight, *first.bn.fold())
        for layer in self.layers.layers[1:]:
            x = layer(x)
        return x
