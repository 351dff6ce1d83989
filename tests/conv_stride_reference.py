"""The reference of the downsampling layers' launches (is_conv_bn_stride, instance_stixels_core.h f19), independent of
the kernel and built on tests/conv_bn_reference.py: torch.nn.functional.conv2d on the CPU in float64 of the half-rounded
operands with stride = stride and padding = 1 (3x3) or 0 (1x1), the same convolution of the absolute values, and
conv_bn_reference's three-step epilogue and tolerance unchanged -- the bound |scale| taps channels_in 2^-23 sum|w x| +
ulp(pre) [+ ulp(prerelu)] counts the terms of one output element and does not depend on the stride.  Results are cached
per case and handed out read-only."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import conv3x3_reference as cr
import conv_bn_reference as cb

DTYPES = cb.DTYPES
KERNELS = cb.KERNELS
STRIDE = 2

# (n, channels_in, channels_out, rows_in, cols_in), all at stride 2; each runs as 3x3 and as 1x1
SHAPES = [
    (2, 16, 32, 5, 7),            # odd extents (the bottom / right padding is read); the phantom channel tile; a batch
    (1, 32, 64, 16, 64),          # even extents, exactly one full output tile, the last input column / row never padded
    (1, 16, 32, 17, 65),          # output 9 x 33: ragged tiles both ways, a halo that crosses the far image edge
    (3, 64, 128, 2, 1),           # a one-column image, output 1 x 1; layer4's channel pair
    (1, 16, 32, 1, 1),            # the smallest image
    (1, 32, 96, 18, 70),          # channels_out = 32 mod 64 with two channel groups and three column tiles
    (1, 64, 64, 15, 66),          # odd rows with even cols; layer3's second channel count
    (1, 128, 128, 16, 64),        # layer4's width, eight chunks
]
SHAPE_IDS = ["%dx%d-%dx%dx%d-s2" % s for s in SHAPES]


def out_extents(rows_in, cols_in, stride=STRIDE):
    """The contract's output extents: ceil(. / stride)."""
    return (rows_in + stride - 1) // stride, (cols_in + stride - 1) // stride


def conv64(x64, w64, kernel, stride=STRIDE):
    """(a, A): the strided convolution of float64 operands (dilation 1) and that of their absolute values."""
    assert tuple(w64.shape[2:]) == (kernel, kernel) and kernel in KERNELS
    pad = 1 if kernel == 3 else 0
    return F.conv2d(x64, w64, stride=stride, padding=pad), F.conv2d(x64.abs(), w64.abs(), stride=stride, padding=pad)


def reference(x, w, scale, shift, kernel, dtype, residual=None, relu=True, stride=STRIDE):
    """fp32 arrays in (w: [co][ci][kernel][kernel]; residual: the OUTPUT's shape, or None); dict(ref, A, tol, pre,
    prerelu) of float64 arrays for the operands rounded to `dtype` (None: not rounded)."""
    a, A = conv64(cb._operand(x, dtype), cb._operand(w, dtype), kernel, stride)
    res = None if residual is None else cb._operand(residual, dtype)
    assert res is None or tuple(res.shape) == tuple(a.shape)
    pre, prerelu, ref = cb.epilogue64(a, scale, shift, res, relu)
    tol = cb.tolerance(pre, prerelu, A, scale, kernel * kernel * np.asarray(x).shape[1], residual is not None)
    return dict(ref=ref.numpy(), A=A.numpy(), tol=tol, pre=pre.numpy(), prerelu=prerelu.numpy())


def _draw(s, kernel, seed, exact):
    n, cin, cout, H, W = SHAPES[s]
    Ho, Wo = out_extents(H, W)
    rng = np.random.default_rng(seed + 10 * s + kernel)
    if exact:
        x = rng.integers(0, 4, (n, cin, H, W)).astype(np.float32)
        m = rng.integers(-255, 256, (cout, cin, kernel, kernel)).astype(np.float64)
        w = (m / 256.0 * (1.0 + 2.0 ** -13)).astype(np.float32)
        scale = rng.choice(np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], np.float32), cout)
        shift = rng.integers(-4, 5, cout).astype(np.float32)
        res = rng.integers(-8, 9, (n, cout, Ho, Wo)).astype(np.float32)
        return cb._frozen(dict(x=x, w=w, m=m, scale=scale, shift=shift, res=res))
    x = np.abs(rng.standard_normal((n, cin, H, W))).astype(np.float32)
    w = (rng.standard_normal((cout, cin, kernel, kernel)) * np.sqrt(2.0 / (kernel * kernel * cout))).astype(np.float32)
    scale = (rng.uniform(0.5, 2.0, cout) * rng.choice([-1.0, 1.0], cout)).astype(np.float32)
    shift = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    res = rng.standard_normal((n, cout, Ho, Wo)).astype(np.float32)
    return cb._frozen(dict(x=x, w=w, scale=scale, shift=shift, res=res))


@functools.lru_cache(maxsize=None)
def exact_inputs(s, kernel):
    """conv_bn_reference.exact_inputs' family at these shapes (the residual has the output's shape): features in
    {0..3}, weights (m / 256)(1 + 2^-13), scale in {+-1/2, +-1, +-2}, integer shift in [-4, 4], integer residual in
    [-8, 8].  A strided output sums a subset of the terms of a stride-1 one, so every partial sum stays a multiple of
    2^-8 below 2^14 and the arithmetic exact in fp32 in any order."""
    return _draw(s, kernel, 5000, True)


@functools.lru_cache(maxsize=None)
def _exact_conv(s, kernel):
    c = exact_inputs(s, kernel)
    return conv64(torch.from_numpy(c["x"].astype(np.float64)), torch.from_numpy(c["m"] / 256.0), kernel)


@functools.lru_cache(maxsize=None)
def exact_reference(s, kernel, with_residual, relu=True):
    """The float64 reference of exact_inputs(s, kernel); the same for both half dtypes, which hold these operands
    exactly (tests/test_conv_stride_cpu.py checks that)."""
    c, (a, A) = exact_inputs(s, kernel), _exact_conv(s, kernel)
    res = torch.from_numpy(c["res"].astype(np.float64)) if with_residual else None
    pre, prerelu, ref = cb.epilogue64(a, c["scale"], c["shift"], res, relu)
    return cb._frozen(dict(ref=ref.numpy(), A=A.numpy(), pre=pre.numpy(), prerelu=prerelu.numpy()))


@functools.lru_cache(maxsize=None)
def random_inputs(s, kernel):
    """conv_bn_reference.random_inputs' family: features |N(0, 1)|, weights N(0, sqrt(2 / (taps channels_out))), scale
    in +-[0.5, 2], shift N(0, 0.1), residual N(0, 1) of the output's shape; fp32."""
    return _draw(s, kernel, 6000, False)


@functools.lru_cache(maxsize=None)
def _random_conv(s, kernel, dtype):
    c = random_inputs(s, kernel)
    return conv64(cr.round_half(c["x"], dtype), cr.round_half(c["w"], dtype), kernel)


@functools.lru_cache(maxsize=None)
def random_reference(s, kernel, dtype, with_residual, relu=True):
    c, (a, A) = random_inputs(s, kernel), _random_conv(s, kernel, dtype)
    res = cr.round_half(c["res"], dtype) if with_residual else None
    pre, prerelu, ref = cb.epilogue64(a, c["scale"], c["shift"], res, relu)
    tol = cb.tolerance(pre, prerelu, A, c["scale"], kernel * kernel * SHAPES[s][1], with_residual)
    return cb._frozen(dict(ref=ref.numpy(), A=A.numpy(), tol=tol, pre=pre.numpy(), prerelu=prerelu.numpy()))
