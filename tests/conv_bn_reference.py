"""The reference of the residual blocks' launches (is_conv_bn, instance_stixels_core.h f18), independent of the kernel
and built on tests/conv3x3_reference.py: torch.nn.functional.conv2d on the CPU in float64 of the half-rounded operands
(3x3 with padding = dilation, or 1x1), the same convolution of the absolute values, and the three-step epilogue in
float64: scale * a + shift, + residual, max(., 0).  Results are cached per case and handed out read-only."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import conv3x3_reference as cr

DTYPES = cr.DTYPES
KERNELS = (3, 1)

# (n, channels_in, channels_out, rows8, cols8, dilation); a 1x1 case runs the same row with dilation 1
SHAPES = cr.SHAPES[:5] + [
    (1, 32, 96, 9, 33, 2),        # channels_out = 32 mod 64 (a phantom channel tile) with a ragged column tile
    (1, 128, 256, 16, 32, 2),     # layer5's channel pair
    (1, 256, 512, 16, 32, 4),     # layer6's channel pair
]
SHAPE_IDS = ["%dx%d-%dx%dx%d-d%d" % s for s in SHAPES]


def dilation_of(s, kernel):
    return SHAPES[s][5] if kernel == 3 else 1


def _operand(a, dtype):
    """fp32 values rounded to the half dtype as float64; dtype None: the values themselves in float64."""
    return torch.from_numpy(np.asarray(a, np.float64)) if dtype is None else cr.round_half(a, dtype)


def conv64(x64, w64, kernel, dilation):
    """(a, A): the convolution of float64 operands and that of their absolute values."""
    if kernel == 3:
        return cr.conv64(x64, w64, dilation)
    assert kernel == 1 and tuple(w64.shape[2:]) == (1, 1)
    return F.conv2d(x64, w64), F.conv2d(x64.abs(), w64.abs())


def epilogue64(a, scale, shift, residual64, relu):
    """(pre, prerelu, ref) in float64: scale[co] * a + shift[co]; + residual; max(., 0) with relu."""
    pre = cr.epilogue64(a, scale, shift, relu=False)
    prerelu = pre if residual64 is None else pre + residual64
    return pre, prerelu, (torch.clamp_min(prerelu, 0.0) if relu else prerelu)


def _ulp32(v64):
    return np.spacing(np.abs(v64.numpy()).astype(np.float32)).astype(np.float64)


def tolerance(pre, prerelu, A, scale, terms, with_residual):
    """|scale| * terms * 2^-23 * A + ulp_fp32(pre) [+ ulp_fp32(prerelu) with a residual], terms = taps * channels_in:
    f17's bound (the exact products summed in any order, each addition off by at most 2^-23 relative; the fmaf's
    rounding) plus the rounding of the fp32 addition of the residual, whose widening is exact.  A full ulp stands
    where the rounding error is half of one, which covers a value next to a binade boundary; ReLU is 1-Lipschitz."""
    sc = torch.from_numpy(np.abs(np.asarray(scale, np.float64))).view(1, -1, 1, 1)
    tol = (sc * (terms * 2.0 ** -23) * A).numpy() + _ulp32(pre)
    return tol + _ulp32(prerelu) if with_residual else tol


def reference(x, w, scale, shift, kernel, dilation, dtype, residual=None, relu=True):
    """fp32 arrays in (w: [co][ci][kernel][kernel]; residual: [n][co][rows][cols] or None); dict(ref, A, tol, pre,
    prerelu) of float64 arrays for the operands rounded to `dtype` (None: not rounded)."""
    w = np.asarray(w)
    assert w.ndim == 4 and w.shape[2] == w.shape[3] == kernel
    a, A = conv64(_operand(x, dtype), _operand(w, dtype), kernel, dilation)
    res = None if residual is None else _operand(residual, dtype)
    pre, prerelu, ref = epilogue64(a, scale, shift, res, relu)
    tol = tolerance(pre, prerelu, A, scale, kernel * kernel * np.asarray(x).shape[1], residual is not None)
    return dict(ref=ref.numpy(), A=A.numpy(), tol=tol, pre=pre.numpy(), prerelu=prerelu.numpy())


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def exact_inputs(s, kernel):
    """f17's exact inputs extended: features integers in {0..3}, weights (m / 256)(1 + 2^-13) with integer |m| <= 255
    (the pack call must round them back to m / 256), scale in {+-1/2, +-1, +-2}, integer shift in [-4, 4], integer
    residual in [-8, 8].  Products are multiples of 2^-8 and every partial sum is at most 9 * 512 * 3 = 13824 < 2^14
    in magnitude; scaled, a multiple of 2^-9 of at most 27648, with shift and residual at most 27660 < 2^15: 24 bits,
    exact in fp32 in any order, up to channels_in = 512."""
    n, cin, cout, H, W, d = SHAPES[s]
    rng = np.random.default_rng(3000 + 10 * s + kernel)
    x = rng.integers(0, 4, (n, cin, H, W)).astype(np.float32)
    m = rng.integers(-255, 256, (cout, cin, kernel, kernel)).astype(np.float64)
    w = (m / 256.0 * (1.0 + 2.0 ** -13)).astype(np.float32)
    scale = rng.choice(np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], np.float32), cout)
    shift = rng.integers(-4, 5, cout).astype(np.float32)
    res = rng.integers(-8, 9, (n, cout, H, W)).astype(np.float32)
    return _frozen(dict(x=x, w=w, m=m, scale=scale, shift=shift, res=res))


@functools.lru_cache(maxsize=None)
def _exact_conv(s, kernel):
    c = exact_inputs(s, kernel)
    return conv64(torch.from_numpy(c["x"].astype(np.float64)), torch.from_numpy(c["m"] / 256.0), kernel,
                  dilation_of(s, kernel))


@functools.lru_cache(maxsize=None)
def exact_reference(s, kernel, with_residual, relu=True):
    """The float64 reference of exact_inputs(s, kernel); the same for both half dtypes, which hold these operands
    exactly (tests/test_conv_bn_cpu.py checks that)."""
    c, (a, A) = exact_inputs(s, kernel), _exact_conv(s, kernel)
    res = torch.from_numpy(c["res"].astype(np.float64)) if with_residual else None
    pre, prerelu, ref = epilogue64(a, c["scale"], c["shift"], res, relu)
    return _frozen(dict(ref=ref.numpy(), A=A.numpy(), pre=pre.numpy(), prerelu=prerelu.numpy()))


@functools.lru_cache(maxsize=None)
def random_inputs(s, kernel):
    """Features |N(0, 1)|, weights N(0, sqrt(2 / (taps channels_out))) (the reference's init, drn.py:191-194), scale
    in +-[0.5, 2], shift N(0, 0.1), residual N(0, 1); fp32."""
    n, cin, cout, H, W, d = SHAPES[s]
    rng = np.random.default_rng(4000 + 10 * s + kernel)
    x = np.abs(rng.standard_normal((n, cin, H, W))).astype(np.float32)
    w = (rng.standard_normal((cout, cin, kernel, kernel)) * np.sqrt(2.0 / (kernel * kernel * cout))).astype(np.float32)
    scale = (rng.uniform(0.5, 2.0, cout) * rng.choice([-1.0, 1.0], cout)).astype(np.float32)
    shift = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    res = rng.standard_normal((n, cout, H, W)).astype(np.float32)
    return _frozen(dict(x=x, w=w, scale=scale, shift=shift, res=res))


@functools.lru_cache(maxsize=None)
def _random_conv(s, kernel, dtype):
    c = random_inputs(s, kernel)
    return conv64(cr.round_half(c["x"], dtype), cr.round_half(c["w"], dtype), kernel, dilation_of(s, kernel))


@functools.lru_cache(maxsize=None)
def random_reference(s, kernel, dtype, with_residual, relu=True):
    c, (a, A) = random_inputs(s, kernel), _random_conv(s, kernel, dtype)
    res = cr.round_half(c["res"], dtype) if with_residual else None
    pre, prerelu, ref = epilogue64(a, c["scale"], c["shift"], res, relu)
    tol = tolerance(pre, prerelu, A, c["scale"], kernel * kernel * SHAPES[s][1], with_residual)
    return _frozen(dict(ref=ref.numpy(), A=A.numpy(), tol=tol, pre=pre.numpy(), prerelu=prerelu.numpy()))


# ---- BasicBlock-shaped modules for the tests of cnn.ResidualBlock ----

def batchnorm(channels, seed):
    """A BatchNorm2d with statistics as after training."""
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm2d(channels)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(channels, generator=g) * 0.2)
        bn.running_var.copy_(torch.rand(channels, generator=g) + 0.5)
        bn.weight.copy_(torch.randn(channels, generator=g))
        bn.bias.copy_(torch.randn(channels, generator=g) * 0.1)
    return bn


class Block(torch.nn.Module):
    """The attributes and the forward of the reference's BasicBlock (drn.py:54-87), written from its description."""

    def __init__(self, cin, cout, dilation=(2, 2), downsample=False, residual=True, stride=1, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.conv1 = torch.nn.Conv2d(cin, cout, 3, stride=stride, padding=dilation[0], dilation=dilation[0], bias=False)
        self.bn1 = batchnorm(cout, seed + 1)
        self.conv2 = torch.nn.Conv2d(cout, cout, 3, padding=dilation[1], dilation=dilation[1], bias=False)
        self.bn2 = batchnorm(cout, seed + 2)
        self.downsample = torch.nn.Sequential(torch.nn.Conv2d(cin, cout, 1, stride=stride, bias=False),
                                              batchnorm(cout, seed + 3)) if downsample else None
        self.residual = residual
        with torch.no_grad():
            for conv in [self.conv1, self.conv2] + ([self.downsample[0]] if downsample else []):
                k = conv.kernel_size[0]
                conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / (k * k * cout)) ** 0.5)

    def forward(self, x):
        out = torch.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        if self.residual:
            out = out + (self.downsample(x) if self.downsample is not None else x)
        return torch.relu(out)
