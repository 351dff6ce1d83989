"""The tail of the reference's backbone on the device (f17): layer7 and layer8 of the DRN (tools/CNN_training/
models/drn.py:181-185, each an nn.Sequential(Conv2d 3x3 dilated without bias, BatchNorm2d, ReLU) built by
_make_conv_layers, drn.py:223-233) and the head `seg` behind them, as three launches of the C ABI with nothing in
between: core.conv3x3_bn_relu twice, core.segmentation_head once.  Inference only: BatchNorm is folded from its running
statistics, nothing here is differentiable.  torch owns the memory and the stream; every value comes from the library's
kernels (there is no fall-back to torch's convolution)."""
import torch

from . import core


def fold_batchnorm(bn):
    """An eval-mode BatchNorm2d as one fp32 (scale, shift) per channel: scale = weight / sqrt(running_var + eps),
    shift = bias - running_mean * scale, computed in float64 and rounded once each.  A module without affine
    parameters counts as weight 1, bias 0.  Raises on a module in training mode (its batch statistics are not a
    function of the module) and on one without running statistics."""
    if not isinstance(bn, torch.nn.modules.batchnorm._BatchNorm):
        raise core.CoreError(f"fold_batchnorm takes a BatchNorm module, not {type(bn).__name__}")
    if bn.training:
        raise core.CoreError("fold_batchnorm folds the running statistics: put the module into eval() mode first")
    if bn.running_mean is None or bn.running_var is None:
        raise core.CoreError("the BatchNorm module tracks no running statistics")
    with torch.no_grad():
        mean, var = bn.running_mean.detach().double().cpu(), bn.running_var.detach().double().cpu()
        weight = bn.weight.detach().double().cpu() if bn.weight is not None else torch.ones_like(mean)
        bias = bn.bias.detach().double().cpu() if bn.bias is not None else torch.zeros_like(mean)
        scale = weight / torch.sqrt(var + float(bn.eps))
        shift = bias - mean * scale
        return scale.float(), shift.float()


class ConvBnRelu:
    """One layer of the tail: the packed weights of `conv` in `dtype` and the fold of `bn`, on `device`.  conv must be
    the reference's: 3x3, stride 1, padding = dilation (the same in both directions), one group, no bias."""

    def __init__(self, conv, bn, dtype=torch.bfloat16, relu=True, device=0):
        d = conv.dilation[0]
        if tuple(conv.kernel_size) != (3, 3) or tuple(conv.stride) != (1, 1) or tuple(conv.dilation) != (d, d) or \
                tuple(conv.padding) != (d, d) or conv.groups != 1 or conv.bias is not None or \
                getattr(conv, "padding_mode", "zeros") != "zeros":
            raise core.CoreError("conv must be Conv2d(kernel_size=3, stride=1, padding=dilation, groups=1, bias=False)")
        if bn.num_features != conv.out_channels:
            raise core.CoreError(f"bn has {bn.num_features} channels, conv {conv.out_channels}")
        dev = torch.device("cuda", device) if not isinstance(device, torch.device) else device
        self.dilation, self.relu, self.dtype = int(d), bool(relu), dtype
        self.packed = core.conv3x3_pack_weights(conv.weight.detach().to(dev), dtype)
        scale, shift = fold_batchnorm(bn)
        self.scale, self.shift = scale.to(dev), shift.to(dev)

    def __call__(self, features, out_dtype=None):
        return core.conv3x3_bn_relu(features, self.packed, self.scale, self.shift, self.dilation, relu=self.relu,
                                    out_dtype=out_dtype)


def _conv_bn_relu_of(layer, name):
    mods = list(layer)
    if len(mods) != 3 or not isinstance(mods[0], torch.nn.Conv2d) or not isinstance(mods[1], torch.nn.BatchNorm2d) \
            or not isinstance(mods[2], torch.nn.ReLU):
        raise core.CoreError(f"{name} must be nn.Sequential(Conv2d, BatchNorm2d, ReLU), as _make_conv_layers builds it")
    return mods[0], mods[1]


class DrnTail:
    """layer7 -> layer8 -> seg -> (-log_softmax, FlipAndPad): the output of the reference's layer6 in, the DP's input
    out.  layer7, layer8: the reference's two nn.Sequential(Conv2d, BatchNorm2d, ReLU), in eval mode; seg: its 1x1
    Conv2d with bias (DRNDownsampled.py:80-85).  The features between the layers stay in `dtype`; the head widens them
    to fp32 exactly.  clamp = (channel, lo, hi) as core.segmentation_head takes it."""

    def __init__(self, layer7, layer8, seg, n_classes, rows_power2_segmentation, clamp=None, dtype=torch.bfloat16,
                 device=0):
        self.layers = [ConvBnRelu(*_conv_bn_relu_of(layer, name), dtype=dtype, device=device)
                       for layer, name in ((layer7, "layer7"), (layer8, "layer8"))]
        if tuple(seg.kernel_size) != (1, 1) or seg.bias is None or seg.in_channels != layer8[0].out_channels:
            raise core.CoreError("seg must be a 1x1 Conv2d with bias on layer8's channels")
        dev = self.layers[0].packed.device
        self.weight = seg.weight.detach().to(device=dev, dtype=torch.float32).reshape(seg.out_channels, -1).contiguous()
        self.bias = seg.bias.detach().to(device=dev, dtype=torch.float32).contiguous()
        self.n_classes, self.p2s, self.clamp, self.dtype = int(n_classes), int(rows_power2_segmentation), clamp, dtype

    @torch.no_grad()
    def forward(self, features, want_cnn_out=False):
        """features: layer6's output [n][C][rows8][cols8] on the device; any other floating dtype than the tail's is
        converted first.  Returns the int32 DP input [n][cols8][channels][rows_power2_segmentation], and with
        want_cnn_out the float32 network output [n][channels][rows8][cols8] behind it."""
        x = features if features.dtype == self.dtype else features.to(self.dtype)
        for layer in self.layers:
            x = layer(x)
        return core.segmentation_head(x, self.weight, self.bias, self.n_classes, self.p2s, want_cnn_out=want_cnn_out,
                                      clamp=self.clamp)

    __call__ = forward
