"""The reference of the backward pass of conv + BatchNorm (+ residual) (+ ReLU) at stride 2 (is_conv_bn_stride_backward,
instance_stixels_core.h f22), built on tests/conv_backward_reference.py: the masked gradient, the scaled weight and the
float64 autograd are that file's; G and dX are torch float64 on the CPU (torch.nn.grad.conv2d_weight / conv2d_input with
stride = 2) of the half-rounded operands as the contract names them, and the same contractions of the absolute values,
which the bounds scale with.  Everything behind gh takes gh as an argument, as there."""
import functools

import numpy as np
import torch
import torch.nn.grad as G

import conv3x3_reference as cr
import conv_backward_reference as cbr

DTYPES = cbr.DTYPES
KERNELS = cbr.KERNELS
BAND = 8       # IS_CONV_BACKWARD_STRIDE_BAND; tests/test_conv_stride_backward_cpu.py checks it against the header and the binding

# (n, channels_in, channels_out, rows_in, cols_in); 3x3 (padding 1) and 1x1 run the same row, stride 2, dilation 1
SHAPES = [
    (1, 32, 32, 2, 2),                     # one output pixel
    (2, 32, 32, 1, 40),                    # a single-row image
    (2, 32, 32, 37, 1),                    # a single-column image
    (1, 32, 64, 17, 65),                   # odd extents: the padding tap is read; 33 output columns, a second segment of one
    (1, 96, 64, 18, 66),                   # even extents: it is never read; channels_in = 32 mod 64
    (2, 64, 128, 12, 63),                  # cols_out 32 whose last kx = 2 tap falls outside
    (3, 32, 32, 2 * BAND + 1, 33),         # a second chunk of one row
    (3, 32, 32, 2 * BAND - 1, 64),         # exactly one full chunk
    (1, 16, 32, 9, 33),                    # layer2's channel count: dW, dscale and dshift only; dX refused
]
SHAPE_IDS = ["%dx%d-%dx%dx%d" % s for s in SHAPES]


def out_extents(s):
    return (SHAPES[s][3] + 1) // 2, (SHAPES[s][4] + 1) // 2


def terms_chunk(Ho, Wo):
    """The products of the largest chunk's accumulator: its OUTPUT rows times the row rounded up to whole K steps of
    16 (no column split)."""
    return min(BAND, Ho) * ((Wo + 15) // 16 * 16)


def taps_of_class(Hi, Wi, kernel):
    """[Hi][Wi]: the taps that reach an element of dX -- 1, 2, 2, 4 by (row, column) parity at kernel 3; 1 at kernel 1
    (only (even, even) elements have it; the others are sums of nothing)."""
    if kernel == 1:
        return np.ones((Hi, Wi))
    r, c = 1 + (np.arange(Hi) & 1), 1 + (np.arange(Wi) & 1)
    return (r[:, None] * c[None, :]).astype(np.float64)


def backward(x, w, scale, gh, kernel, dtype, add=None):
    """conv_backward_reference.backward at stride 2, dilation 1: x [n][ci][Hi][Wi], gh [n][co][Ho][Wo].  The bounds are
    that function's with
      dX      terms = taps_of_class * channels_out (the taps that reach the element's parity class);
      Gsum    terms_chunk = min(BAND, rows_out) * ceil16(cols_out), chunks = n * ceil(rows_out / BAND);
      dshift  over n * rows_out * cols_out."""
    x64, wh64 = cr.round_half(x, dtype), cr.round_half(w, dtype)
    g64 = gh.double() if torch.is_tensor(gh) else cbr._t64(gh)
    n, cin, Hi, Wi = x64.shape
    cout, taps = wh64.shape[0], kernel * kernel
    Ho, Wo = g64.shape[2:]
    kw = dict(stride=2, padding=1 if kernel == 3 else 0)
    sc = cbr._t64(scale)
    Gsum = G.conv2d_weight(x64, wh64.shape, g64, **kw)
    Gabs = G.conv2d_weight(x64.abs(), wh64.shape, g64.abs(), **kw)
    ws = cbr.scaled_weight(w, scale, dtype)
    dx_pre = G.conv2d_input(x64.shape, ws, g64, **kw)
    dx_abs = G.conv2d_input(x64.shape, ws.abs(), g64.abs(), **kw)
    dx = dx_pre if add is None else dx_pre + cr.round_half(add, dtype)
    chunks = n * ((Ho + BAND - 1) // BAND)
    tol_G = (terms_chunk(Ho, Wo) * 2.0 ** -23 + chunks * 2.0 ** -53) * Gabs
    dw = sc.view(-1, 1, 1, 1) * Gsum
    dscale = (wh64 * Gsum).sum((1, 2, 3))
    dshift = g64.sum((0, 2, 3))
    tol_dx = (taps_of_class(Hi, Wi, kernel) * cout * 2.0 ** -23) * dx_abs.numpy() + cbr._ulp32(dx_pre.numpy())
    if add is not None:
        tol_dx = tol_dx + cbr._ulp32(dx.numpy())
    return dict(
        dx=dx.numpy(), G=Gsum.numpy(), dw=dw.numpy(), dscale=dscale.numpy(), dshift=dshift.numpy(), tol_dx=tol_dx,
        tol_G=tol_G.numpy(), tol_dw=(sc.abs().view(-1, 1, 1, 1) * tol_G).numpy() + cbr._ulp32(dw.numpy()),
        tol_dscale=((wh64.abs() * tol_G).sum((1, 2, 3)) + cin * taps * 2.0 ** -53 * (wh64 * Gsum).abs().sum((1, 2, 3))).numpy()
        + cbr._ulp32(dscale.numpy()),
        tol_dshift=(n * Ho * Wo * 2.0 ** -53 * g64.abs().sum((0, 2, 3))).numpy() + cbr._ulp32(dshift.numpy()))


@functools.lru_cache(maxsize=None)
def exact_inputs(s, kernel):
    """conv_backward_reference.exact_inputs' family at this file's shapes: x integers in {0..3}, w = (m / 256)(1 + 2^-13),
    scale in {+-1/2, +-1, +-2}, integer shift, residual, dY in [-2, 2] and features_add in [-8, 8]; res and dy have the
    OUTPUT's extents, add the input's.  The claims of exactness are that docstring's, with a chunk of at most BAND *
    cols_out products (tests/test_conv_stride_backward_cpu.py checks the shapes)."""
    n, cin, cout, Hi, Wi = SHAPES[s]
    Ho, Wo = out_extents(s)
    rng = np.random.default_rng(7000 + 10 * s + kernel)
    x = rng.integers(0, 4, (n, cin, Hi, Wi)).astype(np.float32)
    m = rng.integers(-255, 256, (cout, cin, kernel, kernel)).astype(np.float64)
    w = (m / 256.0 * (1.0 + 2.0 ** -13)).astype(np.float32)
    scale = rng.choice(np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], np.float32), cout)
    shift = rng.integers(-4, 5, cout).astype(np.float32)
    res = rng.integers(-8, 9, (n, cout, Ho, Wo)).astype(np.float32)
    dy = rng.integers(-2, 3, (n, cout, Ho, Wo)).astype(np.float32)
    add = rng.integers(-8, 9, (n, cin, Hi, Wi)).astype(np.float32)
    return cbr._frozen(dict(x=x, w=w, m=m, scale=scale, shift=shift, res=res, dy=dy, add=add))


@functools.lru_cache(maxsize=None)
def random_inputs(s, kernel):
    """conv_backward_reference.random_inputs' family at this file's shapes."""
    n, cin, cout, Hi, Wi = SHAPES[s]
    Ho, Wo = out_extents(s)
    rng = np.random.default_rng(8000 + 10 * s + kernel)
    x = np.abs(rng.standard_normal((n, cin, Hi, Wi))).astype(np.float32)
    w = (rng.standard_normal((cout, cin, kernel, kernel)) * np.sqrt(2.0 / (kernel * kernel * cout))).astype(np.float32)
    scale = (rng.uniform(0.5, 2.0, cout) * rng.choice([-1.0, 1.0], cout)).astype(np.float32)
    shift = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    res = rng.standard_normal((n, cout, Ho, Wo)).astype(np.float32)
    dy = rng.standard_normal((n, cout, Ho, Wo)).astype(np.float32)
    add = rng.standard_normal((n, cin, Hi, Wi)).astype(np.float32)
    return cbr._frozen(dict(x=x, w=w, scale=scale, shift=shift, res=res, dy=dy, add=add))


def autograd64(x, w, scale, shift, res, dy, kernel, relu=True):
    """float64 torch.autograd of relu(scale * conv2d(x, w, stride=2) + shift + res) against the upstream gradient dy:
    dict(out, dx, dw, dscale, dshift, dres)."""
    leaf = lambda a: cbr._t64(a).requires_grad_(True)
    xt, wt, sc, sh = leaf(x), leaf(w), leaf(scale), leaf(shift)
    rt = leaf(res) if res is not None else None
    v = sc.view(1, -1, 1, 1) * torch.nn.functional.conv2d(xt, wt, stride=2, padding=1 if kernel == 3 else 0) + sh.view(1, -1, 1, 1)
    if rt is not None:
        v = v + rt
    out = torch.relu(v) if relu else v
    out.backward(cbr._t64(dy))
    return dict(out=out.detach().numpy(), dx=xt.grad.numpy(), dw=wt.grad.numpy(), dscale=sc.grad.numpy(),
                dshift=sh.grad.numpy(), dres=rt.grad.numpy() if rt is not None else None)
