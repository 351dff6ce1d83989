"""The tail of the reference's backbone on the device (f17): layer7 and layer8 of the DRN (tools/CNN_training/
models/drn.py:181-185, each an nn.Sequential(Conv2d 3x3 dilated without bias, BatchNorm2d, ReLU) built by
_make_conv_layers, drn.py:223-233) and the head `seg` behind them, as three launches of the C ABI with nothing in
between: core.conv_bn twice (with kernel 3 and no residual, the bytes of f17's core.conv3x3_bn_relu), then
core.segmentation_head once.  Inference only: BatchNorm is folded from its running statistics, nothing here is
differentiable.  torch owns the memory and the stream; every value comes from the library's kernels (there is no
fall-back to torch's convolution).

f18 puts the residual blocks of layer5 and layer6 in front of it (BasicBlock, drn.py:54-87, built by _make_layer,
drn.py:199-221, as drn.py:168-172): ResidualBlock is two launches of core.conv_bn, three with a downsample, and
DrnDilated is layer5 -> layer6 -> DrnTail, the output of layer4 in and the DP's input out.

Every convolution here is one ConvBn: the packed weights, the folded BatchNorm and the launch's kernel, dilation and
relu.  The tail's ConvBnRelu is a ConvBn built from (Conv2d, BatchNorm2d); a ResidualBlock holds two or three.

f19 puts the downsampling layers in front of that: layer2 (one stride-2 conv + BN + ReLU, drn.py:161-163) and the
BasicBlocks of layer3 and layer4 (drn.py:164-167), whose first block has stride 2 in conv1 and in the downsample.  A
ConvBn carries its stride and launches core.conv_bn_stride (at stride 1 the bytes of core.conv_bn); the classes that
accept stride 2 are StridedConvBnRelu and StridedResidualBlock, which differ from ConvBnRelu and ResidualBlock in the
strides they allow and in nothing else.  DrnDownsampling is layer2 -> layer3 -> layer4 -> DrnDilated: the output of
layer1 at full resolution in, the DP's input out, 24 launches.

f20 puts the stem in front of that: DrnStem is the table look-up of the image's bytes (input_table: ToTensor +
Normalize + the cast to half), layer0 (7x7, 3 -> 16) and layer1 (3x3, 16 -> 16) in ONE launch of core.stem, and Drn is
DrnStem -> DrnDownsampling: the camera's uint8 image in, the DP's input out, 25 launches for drn_d_22."""
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


def _device(device):
    return device if isinstance(device, torch.device) else torch.device("cuda", device)


def _dilated3x3(conv, name, strides=(1,)):
    """The dilation of `conv` if it is the reference's 3x3: padding = dilation (the same in both directions), one
    group, no bias, and a stride (the same in both directions) out of `strides`; stride 2 needs dilation 1."""
    if not isinstance(conv, torch.nn.Conv2d) or tuple(conv.kernel_size) != (3, 3) or \
            tuple(conv.dilation) != (conv.dilation[0],) * 2 or tuple(conv.padding) != tuple(conv.dilation) or \
            conv.groups != 1 or conv.bias is not None or getattr(conv, "padding_mode", "zeros") != "zeros":
        raise core.CoreError(f"{name} must be Conv2d(kernel_size=3, padding=dilation, groups=1, bias=False)")
    if tuple(conv.stride) not in [(s, s) for s in strides]:
        raise core.CoreError(f"{name} has stride {tuple(conv.stride)}: " +
                             ("only the stride-1 layers (layer5 on) are covered" if tuple(strides) == (1,) else
                              f"only the strides {tuple(strides)} are covered"))
    if conv.stride[0] == 2 and conv.dilation[0] != 1:
        raise core.CoreError(f"{name} has stride 2 with dilation {conv.dilation[0]}: stride 2 needs dilation 1")
    return int(conv.dilation[0])


class ConvBn:
    """A packed convolution and its folded BatchNorm on a device, one launch of core.conv_bn_stride per call (at stride
    1 core.conv_bn's launch and bytes): `weight` is conv.weight [channels_out][channels_in][kernel][kernel], `fold` the
    (scale, shift) of fold_batchnorm.  Nothing is checked here beyond what core.conv_pack_weights checks: the callers
    check and fold first, then build this."""

    def __init__(self, weight, fold, kernel, dilation, relu, dtype, dev, stride=1):
        self.kernel, self.dilation, self.relu, self.dtype = int(kernel), int(dilation), bool(relu), dtype
        self.stride = int(stride)
        self.packed = core.conv_pack_weights(weight.detach().to(dev), dtype)
        self.scale, self.shift = fold[0].to(dev), fold[1].to(dev)

    def __call__(self, features, out_dtype=None, residual=None):
        return core.conv_bn_stride(features, self.packed, self.scale, self.shift, self.kernel, self.stride,
                                   self.dilation, residual=residual, relu=self.relu, out_dtype=out_dtype)


class ConvBnRelu(ConvBn):
    """One layer of the tail: the packed weights of `conv` in `dtype` and the fold of `bn`, on `device`.  conv must be
    the reference's: 3x3, stride 1, padding = dilation (the same in both directions), one group, no bias."""

    strides = (1,)     # the strides of conv that the class accepts

    def __init__(self, conv, bn, dtype=torch.bfloat16, relu=True, device=0):
        d = _dilated3x3(conv, "conv", self.strides)
        if bn.num_features != conv.out_channels:
            raise core.CoreError(f"bn has {bn.num_features} channels, conv {conv.out_channels}")
        super().__init__(conv.weight, fold_batchnorm(bn), 3, d, relu, dtype, _device(device), stride=conv.stride[0])


class StridedConvBnRelu(ConvBnRelu):
    """ConvBnRelu for a conv of stride 1 or 2 (layer2 of the reference: stride 2, padding 1, dilation 1)."""

    strides = (1, 2)


def _conv_bn_relu_of(layer, name):
    mods = list(layer)
    if len(mods) != 3 or not isinstance(mods[0], torch.nn.Conv2d) or not isinstance(mods[1], torch.nn.BatchNorm2d) \
            or not isinstance(mods[2], torch.nn.ReLU):
        raise core.CoreError(f"{name} must be nn.Sequential(Conv2d, BatchNorm2d, ReLU), as _make_conv_layers builds it")
    return mods[0], mods[1]


class ResidualBlock:
    """One BasicBlock of the reference (drn.py:54-87) in eval mode: relu(bn1(conv1(x))), then bn2(conv2(.)) with the
    residual -- downsample(x) or x itself -- added in fp32 between the BatchNorm and the ReLU (is_conv_bn's epilogue),
    as 2 launches, or 3 with a downsample.  `block` is any object with the attributes conv1, bn1, conv2, bn2,
    downsample and residual; residual=False (arch C's layer7 / layer8) gives two plain conv + BN + ReLU launches.
    Everything is checked and folded before the weights are packed on `device`."""

    strides = (1,)     # the strides of conv1 (and with it of the downsample) that the class accepts; conv2 has 1

    def __init__(self, block, dtype=torch.bfloat16, device=0):
        if hasattr(block, "conv3"):
            raise core.CoreError("a block with conv3 is a Bottleneck: only BasicBlock is covered")
        d1, d2 = _dilated3x3(block.conv1, "conv1", self.strides), _dilated3x3(block.conv2, "conv2")
        stride = int(block.conv1.stride[0])
        c_in, c_mid, c_out = block.conv1.in_channels, block.conv1.out_channels, block.conv2.out_channels
        if block.conv2.in_channels != c_mid or block.bn1.num_features != c_mid or block.bn2.num_features != c_out:
            raise core.CoreError("conv1, bn1, conv2 and bn2 disagree on their channels")
        self.residual = bool(block.residual)
        down = block.downsample if self.residual else None      # (the reference computes and drops it otherwise)
        fold1, fold2, fold_down = fold_batchnorm(block.bn1), fold_batchnorm(block.bn2), None
        if down is not None:
            mods = list(down) if isinstance(down, torch.nn.Sequential) else []
            if len(mods) != 2 or not isinstance(mods[0], torch.nn.Conv2d) or not isinstance(mods[1], torch.nn.BatchNorm2d) \
                    or tuple(mods[0].kernel_size) != (1, 1) or mods[0].bias is not None or mods[0].groups != 1 \
                    or tuple(mods[0].padding) != (0, 0) or mods[0].in_channels != c_in or mods[0].out_channels != c_out \
                    or mods[1].num_features != c_out:
                raise core.CoreError("downsample must be nn.Sequential(Conv2d(kernel_size=1, bias=False), BatchNorm2d) "
                                     "from the block's input to its output channels")
            if tuple(mods[0].stride) != (stride, stride):
                raise core.CoreError(f"downsample has stride {tuple(mods[0].stride)}, conv1 {(stride, stride)}: the "
                                     "residual must have the shape of conv2's output")
            fold_down = fold_batchnorm(mods[1])
        elif self.residual and stride != 1:
            raise core.CoreError(f"conv1 has stride {stride} and the block no downsample: the input cannot be the residual")
        elif self.residual and c_in != c_out:
            raise core.CoreError(f"residual=True without a downsample needs equal channels, not {c_in} -> {c_out}")
        dev = _device(device)
        self.dtype = dtype
        self.conv1 = ConvBn(block.conv1.weight, fold1, 3, d1, True, dtype, dev, stride=stride)
        self.conv2 = ConvBn(block.conv2.weight, fold2, 3, d2, True, dtype, dev)
        self.downsample = ConvBn(mods[0].weight, fold_down, 1, 1, False, dtype, dev, stride=stride) \
            if down is not None else None

    @property
    def packed(self):
        """The packed weights of the block's launches: conv1's, conv2's and, if there is one, the downsample's."""
        return [layer.packed for layer in (self.conv1, self.conv2, self.downsample) if layer is not None]

    def __call__(self, x, out_dtype=None):
        """x: [n][channels_in][rows8][cols8] of the block's dtype on its device."""
        y = self.conv1(x)
        res = None
        if self.residual:
            res = self.downsample(x) if self.downsample is not None else x
        return self.conv2(y, out_dtype=out_dtype, residual=res)


class StridedResidualBlock(ResidualBlock):
    """ResidualBlock for a BasicBlock whose conv1 has stride 1 or 2 (the first blocks of layer3 and layer4: stride 2,
    dilation 1).  With stride 2 the block needs a downsample of the same stride -- the residual has the shape of
    conv2's output, ceil(rows / 2) x ceil(cols / 2) -- and conv1 dilation 1; conv2 has stride 1."""

    strides = (1, 2)


def input_table(mean, std, dtype):
    """The [3][256] table of ToTensor + Normalize(mean, std) + the cast to `dtype` (inference.py:109-110, :278):
    ((arange(256, fp32) / 255) - mean[c]) / std[c] in fp32 on the CPU, then .to(dtype).  mean, std: three values each,
    in the order of the image's bytes."""
    if dtype not in (torch.float16, torch.bfloat16):
        raise core.CoreError(f"dtype {dtype} is neither torch.float16 nor torch.bfloat16")
    mean = torch.as_tensor(mean, dtype=torch.float32).reshape(-1).cpu()
    std = torch.as_tensor(std, dtype=torch.float32).reshape(-1).cpu()
    if mean.numel() != 3 or std.numel() != 3:
        raise core.CoreError("mean and std must hold three values each")
    unit = torch.arange(256, dtype=torch.float32) / 255
    return ((unit.view(1, 256) - mean.view(3, 1)) / std.view(3, 1)).to(dtype)


def _stem_conv(layer, name, channels_in, kernel, padding, why_not_three):
    """(conv, bn) of a stem layer: nn.Sequential(Conv2d(channels_in, 16, kernel, stride 1, padding, dilation 1,
    bias=False), BatchNorm2d, ReLU) with exactly three modules."""
    mods = list(layer) if isinstance(layer, torch.nn.Sequential) else None
    if mods is None:
        raise core.CoreError(f"{name} must be an nn.Sequential, not {type(layer).__name__}")
    if any(hasattr(m, "conv1") and hasattr(m, "conv2") for m in mods):
        raise core.CoreError(f"{name} holds a BasicBlock (arch C builds its {name} from blocks): only arch D's "
                             "Conv2d + BatchNorm2d + ReLU stem is covered")
    if len(mods) != 3:
        raise core.CoreError(f"{name} has {len(mods)} modules, not the three of Conv2d + BatchNorm2d + ReLU" + why_not_three)
    conv, bn, relu = mods
    if not isinstance(conv, torch.nn.Conv2d) or not isinstance(bn, torch.nn.BatchNorm2d) or not isinstance(relu, torch.nn.ReLU):
        raise core.CoreError(f"{name} must be nn.Sequential(Conv2d, BatchNorm2d, ReLU)")
    if conv.in_channels != channels_in or conv.out_channels != 16 or tuple(conv.kernel_size) != (kernel, kernel) or \
            tuple(conv.stride) != (1, 1) or tuple(conv.padding) != (padding, padding) or tuple(conv.dilation) != (1, 1) or \
            conv.groups != 1 or getattr(conv, "padding_mode", "zeros") != "zeros":
        raise core.CoreError(f"{name}'s conv must be Conv2d({channels_in}, 16, kernel_size={kernel}, stride=1, "
                             f"padding={padding}, dilation=1, groups=1)")
    if conv.bias is not None:
        raise core.CoreError(f"{name}'s conv has a bias: the reference's has none (bias=False)")
    if bn.num_features != 16:
        raise core.CoreError(f"{name}'s bn has {bn.num_features} channels, its conv 16")
    return conv, bn


class DrnStem:
    """ToTensor + Normalize + half -> layer0 -> layer1 of the reference's drn_d_22 in one launch (core.stem): the uint8
    image [n][rows][cols][3] in, layer1's output [n][16][rows][cols] out.
    layer0: nn.Sequential(Conv2d(3, 16, 7, stride 1, padding 3, bias=False), BatchNorm2d, ReLU) (drn.py:154-159);
    layer1: nn.Sequential(Conv2d(16, 16, 3, stride 1, padding 1, dilation 1, bias=False), BatchNorm2d, ReLU) with
    exactly three modules (drn.py:161-162 with layers[0] == 1), both in eval mode; mean, std: Normalize's, in the order
    of the image's bytes (a BGR caller permutes them and layer0's input channels).  Everything is
    checked and folded before anything is packed on `device`."""

    def __init__(self, layer0, layer1, mean, std, dtype=torch.bfloat16, device=0):
        conv0, bn0 = _stem_conv(layer0, "layer0", 3, 7, 3, "")
        conv1, bn1 = _stem_conv(layer1, "layer1", 16, 3, 1, " (layers[0] > 1 repeats the three: only layers[0] == 1 is covered)")
        fold0, fold1 = fold_batchnorm(bn0), fold_batchnorm(bn1)
        table = input_table(mean, std, dtype)
        dev = _device(device)
        self.dtype = dtype
        self.packed = core.stem_pack_weights(conv0.weight, conv1.weight, dtype, device=dev)
        self.lut = table.to(dev)
        self.fold0 = (fold0[0].to(dev), fold0[1].to(dev))
        self.fold1 = (fold1[0].to(dev), fold1[1].to(dev))

    launches = 1

    @torch.no_grad()
    def forward(self, image, want_mid=False):
        """image: uint8 [n][rows][cols][3] on the device.  Returns layer1's output, with want_mid (out, mid)."""
        return core.stem(image, self.lut, self.packed, *self.fold0, *self.fold1, want_mid=want_mid)

    __call__ = forward


class Drn:
    """DrnStem -> DrnDownsampling: the camera's uint8 image [n][rows][cols][3] in, the DP's input out, in 25 launches
    for drn_d_22 with nothing of torch in between."""

    def __init__(self, layer0, layer1, layer2, layer3, layer4, layer5, layer6, layer7, layer8, seg, n_classes,
                 rows_power2_segmentation, mean, std, clamp=None, dtype=torch.bfloat16, device=0):
        self.stem = DrnStem(layer0, layer1, mean, std, dtype=dtype, device=device)
        self.downsampling = DrnDownsampling(layer2, layer3, layer4, layer5, layer6, layer7, layer8, seg, n_classes,
                                            rows_power2_segmentation, clamp=clamp, dtype=dtype, device=device)
        self.dtype = dtype

    @classmethod
    def from_base(cls, base, seg, n_classes, rows_power2_segmentation, mean, std, clamp=None, dtype=torch.bfloat16,
                  device=0):
        """base: the reference's model.base, the nn.Sequential of the nine children layer0 .. layer8
        (DRNDownsampled.py:77)."""
        layers = list(base)
        if len(layers) != 9:
            raise core.CoreError(f"base has {len(layers)} children, not the nine layer0 .. layer8")
        return cls(*layers, seg, n_classes, rows_power2_segmentation, mean, std, clamp=clamp, dtype=dtype, device=device)

    @property
    def launches(self):
        return self.stem.launches + self.downsampling.launches

    @torch.no_grad()
    def forward(self, image, want_cnn_out=False):
        """image: uint8 [n][rows][cols][3] on the device.  Returns what DrnTail.forward returns."""
        return self.downsampling.forward(self.stem.forward(image), want_cnn_out=want_cnn_out)

    __call__ = forward


class DrnDownsampling:
    """layer2 -> layer3 -> layer4 -> layer5 -> ... -> layer8 -> seg -> (-log_softmax, FlipAndPad): the output of the
    reference's layer1 [n][16][rows][cols] at full resolution in, the DP's input out, in 24 launches for drn_d_22.
    layer2: nn.Sequential(Conv2d(3x3, stride 2, padding 1, bias=False), BatchNorm2d, ReLU); layer3, layer4: sequences
    of BasicBlocks in eval mode (StridedResidualBlock); the rest is DrnDilated's.  rows and cols need not be multiples
    of 8: the extents follow ceil(. / 2) three times, as the reference's do."""

    def __init__(self, layer2, layer3, layer4, layer5, layer6, layer7, layer8, seg, n_classes,
                 rows_power2_segmentation, clamp=None, dtype=torch.bfloat16, device=0):
        self.layer2 = StridedConvBnRelu(*_conv_bn_relu_of(layer2, "layer2"), dtype=dtype, device=device)
        self.blocks = [StridedResidualBlock(b, dtype=dtype, device=device) for layer in (layer3, layer4) for b in layer]
        self.dilated = DrnDilated(layer5, layer6, layer7, layer8, seg, n_classes, rows_power2_segmentation, clamp=clamp,
                                  dtype=dtype, device=device)
        self.dtype = dtype

    @property
    def launches(self):
        """The launches of one forward: one per packed convolution, and the head."""
        blocks = self.blocks + self.dilated.blocks
        return 1 + sum(len(b.packed) for b in blocks) + len(self.dilated.tail.layers) + 1

    @torch.no_grad()
    def forward(self, features, want_cnn_out=False):
        """features: layer1's output [n][16][rows][cols] on the device; any other floating dtype than `dtype` is
        converted first.  Returns what DrnTail.forward returns."""
        x = features if features.dtype == self.dtype else features.to(self.dtype)
        x = self.layer2(x)
        for block in self.blocks:
            x = block(x)
        return self.dilated.forward(x, want_cnn_out=want_cnn_out)

    __call__ = forward


class DrnDilated:
    """layer5 -> layer6 -> layer7 -> layer8 -> seg -> (-log_softmax, FlipAndPad): the output of the reference's layer4
    in, the DP's input out.  layer5, layer6: sequences of BasicBlocks in eval mode (ResidualBlock); the rest is
    DrnTail's.  The features between the launches stay in `dtype`."""

    def __init__(self, layer5, layer6, layer7, layer8, seg, n_classes, rows_power2_segmentation, clamp=None,
                 dtype=torch.bfloat16, device=0):
        self.blocks = [ResidualBlock(b, dtype=dtype, device=device) for layer in (layer5, layer6) for b in layer]
        self.tail = DrnTail(layer7, layer8, seg, n_classes, rows_power2_segmentation, clamp=clamp, dtype=dtype,
                            device=device)
        self.dtype = dtype

    @torch.no_grad()
    def forward(self, features, want_cnn_out=False):
        """features: layer4's output [n][C][rows8][cols8] on the device; any other floating dtype than `dtype` is
        converted first.  Returns what DrnTail.forward returns."""
        x = features if features.dtype == self.dtype else features.to(self.dtype)
        for block in self.blocks:
            x = block(x)
        return self.tail.forward(x, want_cnn_out=want_cnn_out)

    __call__ = forward


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
