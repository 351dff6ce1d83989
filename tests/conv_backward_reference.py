"""The reference of the backward pass of conv + BatchNorm (+ residual) (+ ReLU) (is_conv_bn_backward,
instance_stixels_core.h f21), independent of the kernel and built on tests/conv_bn_reference.py: the masked gradient gh
by numpy / torch's CPU conversion on the rounded operands; G, dX and dshift by torch float64 on the CPU
(torch.nn.grad.conv2d_weight / conv2d_input) of the half-rounded operands as the contract names them, including
round_half(scale * w_half); the same contractions of the absolute values, which the bounds scale with.  Everything
behind gh takes gh as an argument: the GPU tests pin gh bit for bit and everything else on the device's own gh."""
import functools

import numpy as np
import torch
import torch.nn.grad as G

import conv3x3_reference as cr
import conv_bn_reference as cb

DTYPES = cb.DTYPES
KERNELS = cb.KERNELS
BAND = 32      # IS_CONV_BACKWARD_BAND; tests/test_conv_backward_cpu.py checks it against the header and the binding

# (n, channels_in, channels_out, rows8, cols8, dilation); a 1x1 case runs the same row with dilation 1
SHAPES = list(cb.SHAPES) + [
    (1, 96, 64, 9, 33, 2),                 # channels_in = 32 mod 64
    (3, 32, 32, BAND + 1, 33, 1),          # two chunks per image, the second of one row; three images
    (3, 32, 32, 2 * BAND + 5, 33, 2),      # three chunks per image
    (2, 32, 32, 1, 40, 1),                 # a 1-row image
    (2, 32, 32, 37, 1, 2),                 # a 1-column image
]
SHAPE_IDS = ["%dx%d-%dx%dx%d-d%d" % s for s in SHAPES]


def dilation_of(s, kernel):
    return SHAPES[s][5] if kernel == 3 else 1


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))


def masked_gradient(dy, out, relu, dtype):
    """gh as a tensor of the half dtype: round_half(dY) where relu is off or the stored `out` is > 0, else +0.  dy, out:
    arrays or CPU tensors of fp32 or the half dtype."""
    td = DTYPES[dtype]
    gy = torch.tensor(np.asarray(dy)) if not torch.is_tensor(dy) else dy
    gh = gy.to(td)                                              # torch's conversion on the CPU: round to nearest even
    if not relu:
        return gh
    o = torch.tensor(np.asarray(out)) if not torch.is_tensor(out) else out
    return torch.where(o.double() > 0, gh, torch.zeros_like(gh))


def scaled_weight(w, scale, dtype):
    """round_half(scale[co] * w_half[co][ci][tap]) as float64: the product in fp32, rounded once."""
    wh = torch.tensor(np.asarray(w, np.float32)).to(DTYPES[dtype]).float()
    sc = torch.tensor(np.asarray(scale, np.float32)).view(-1, 1, 1, 1)
    return (sc * wh).to(DTYPES[dtype]).double()


def _ulp32(v64):
    return np.spacing(np.abs(np.asarray(v64)).astype(np.float32)).astype(np.float64)


def terms_chunk(H, W):
    """The products of the largest chunk's accumulator: its rows times the row rounded up to whole K steps of 16."""
    return min(BAND, H) * ((W + 15) // 16 * 16)


def backward(x, w, scale, gh, kernel, dilation, dtype, add=None):
    """x, w, scale: fp32 arrays (x and w are rounded to `dtype` here); gh: the masked gradient as a half tensor or an
    array of its values; add: the features_add operand or None.  Returns float64 arrays: the references dx (before the
    final rounding), G, dw, dscale, dshift, and the bounds tol_dx (for the fp32 output), tol_G, tol_dw, tol_dscale,
    tol_dshift.

      dX      f18's bound with terms = taps * channels_out and scale 1: terms 2^-23 sum|wT gh| + ulp_fp32(dx before the
              add) [+ ulp_fp32(dx) with an add].
      Gsum    a chunk's accumulator adds at most terms_chunk exact products, each addition off by at most 2^-23
              relative: terms_chunk 2^-23 sum|gh x| over the chunk; the chunks' bounds add up to the same factor times
              the whole sum.  The binary64 sum of the at most n * bands partials adds (n bands) 2^-53 of it.
      dW      |scale| tol_G + ulp_fp32(dw): the product and the rounding happen once, in binary64 -> fp32.
      dscale  sum |w_half| tol_G + (channels_in taps) 2^-53 sum|w_half G| + ulp_fp32(dscale).
      dshift  (n P) 2^-53 sum|gh| + ulp_fp32(dshift)."""
    x64, wh64 = cr.round_half(x, dtype), cr.round_half(w, dtype)
    g64 = gh.double() if torch.is_tensor(gh) else _t64(gh)
    n, cin, H, W = x64.shape
    cout, taps = wh64.shape[0], kernel * kernel
    pad = dilation if kernel == 3 else 0
    kw = dict(padding=pad, dilation=dilation)
    sc = _t64(scale)
    Gsum = G.conv2d_weight(x64, wh64.shape, g64, **kw)
    Gabs = G.conv2d_weight(x64.abs(), wh64.shape, g64.abs(), **kw)
    ws = scaled_weight(w, scale, dtype)
    dx_pre = G.conv2d_input(x64.shape, ws, g64, **kw)
    dx_abs = G.conv2d_input(x64.shape, ws.abs(), g64.abs(), **kw)
    dx = dx_pre if add is None else dx_pre + cr.round_half(add, dtype)
    chunks = n * ((H + BAND - 1) // BAND)
    tol_G = (terms_chunk(H, W) * 2.0 ** -23 + chunks * 2.0 ** -53) * Gabs
    dw = sc.view(-1, 1, 1, 1) * Gsum
    dscale = (wh64 * Gsum).sum((1, 2, 3))
    dshift = g64.sum((0, 2, 3))
    tol_dx = (taps * cout * 2.0 ** -23) * dx_abs.numpy() + _ulp32(dx_pre.numpy())
    if add is not None:
        tol_dx = tol_dx + _ulp32(dx.numpy())
    return dict(
        dx=dx.numpy(), G=Gsum.numpy(), dw=dw.numpy(), dscale=dscale.numpy(), dshift=dshift.numpy(), tol_dx=tol_dx,
        tol_G=tol_G.numpy(), tol_dw=(sc.abs().view(-1, 1, 1, 1) * tol_G).numpy() + _ulp32(dw.numpy()),
        tol_dscale=((wh64.abs() * tol_G).sum((1, 2, 3)) + cin * taps * 2.0 ** -53 * (wh64 * Gsum).abs().sum((1, 2, 3))).numpy()
        + _ulp32(dscale.numpy()),
        tol_dshift=(n * H * W * 2.0 ** -53 * g64.abs().sum((0, 2, 3))).numpy() + _ulp32(dshift.numpy()))


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def exact_inputs(s, kernel):
    """conv_bn_reference.exact_inputs' family at this file's shapes, extended with an integer dY in [-2, 2] and an
    integer features_add in [-8, 8].  gh x products are integers of at most 6, a chunk sums at most BAND * cols8 of
    them: below 2^24 while BAND * cols8 * 6 < 2^24 (tests/test_conv_backward_cpu.py checks the shapes).  wT = scale * m /
    256 is a multiple of 2^-9 of at most 2 and exact in both half dtypes, dX sums at most 9 * 512 products of at most
    4: multiples of 2^-9 below 2^15, 24 bits.  So G, dX, dW, dscale and dshift are exact in every order."""
    n, cin, cout, H, W, d = SHAPES[s]
    rng = np.random.default_rng(5000 + 10 * s + kernel)
    x = rng.integers(0, 4, (n, cin, H, W)).astype(np.float32)
    m = rng.integers(-255, 256, (cout, cin, kernel, kernel)).astype(np.float64)
    w = (m / 256.0 * (1.0 + 2.0 ** -13)).astype(np.float32)
    scale = rng.choice(np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], np.float32), cout)
    shift = rng.integers(-4, 5, cout).astype(np.float32)
    res = rng.integers(-8, 9, (n, cout, H, W)).astype(np.float32)
    dy = rng.integers(-2, 3, (n, cout, H, W)).astype(np.float32)
    add = rng.integers(-8, 9, (n, cin, H, W)).astype(np.float32)
    return _frozen(dict(x=x, w=w, m=m, scale=scale, shift=shift, res=res, dy=dy, add=add))


@functools.lru_cache(maxsize=None)
def random_inputs(s, kernel):
    """conv_bn_reference.random_inputs' family at this file's shapes, with dY N(0, 1) and features_add N(0, 1)."""
    n, cin, cout, H, W, d = SHAPES[s]
    rng = np.random.default_rng(6000 + 10 * s + kernel)
    x = np.abs(rng.standard_normal((n, cin, H, W))).astype(np.float32)
    w = (rng.standard_normal((cout, cin, kernel, kernel)) * np.sqrt(2.0 / (kernel * kernel * cout))).astype(np.float32)
    scale = (rng.uniform(0.5, 2.0, cout) * rng.choice([-1.0, 1.0], cout)).astype(np.float32)
    shift = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    res = rng.standard_normal((n, cout, H, W)).astype(np.float32)
    dy = rng.standard_normal((n, cout, H, W)).astype(np.float32)
    add = rng.standard_normal((n, cin, H, W)).astype(np.float32)
    return _frozen(dict(x=x, w=w, scale=scale, shift=shift, res=res, dy=dy, add=add))


def autograd64(x, w, scale, shift, res, dy, kernel, dilation, relu=True, bn=None):
    """float64 torch.autograd of relu(scale * conv2d(x, w) + shift + res) against the upstream gradient dy, all
    operands as given (float64 arrays).  bn = (weight, bias, mean, var, eps): scale and shift are the fold of them, and
    the gradients of weight and bias, (dscale, dshift) sent on through the fold, are returned too.  Returns dict(out, dx, dw, dscale, dshift, dres[,
    dbn_weight, dbn_bias])."""
    leaf = lambda a: _t64(a).requires_grad_(True)
    xt, wt = leaf(x), leaf(w)
    rt = leaf(res) if res is not None else None
    if bn is not None:
        bw, bb = leaf(bn[0]), leaf(bn[1])
        sc_fold = bw / torch.sqrt(_t64(bn[3]) + bn[4])
        sh_fold = bb - _t64(bn[2]) * sc_fold
        sc, sh = sc_fold.detach().clone().requires_grad_(True), sh_fold.detach().clone().requires_grad_(True)
    else:
        sc, sh = leaf(scale), leaf(shift)
    pad = dilation if kernel == 3 else 0
    v = sc.view(1, -1, 1, 1) * torch.nn.functional.conv2d(xt, wt, padding=pad, dilation=dilation) + sh.view(1, -1, 1, 1)
    if rt is not None:
        v = v + rt
    out = torch.relu(v) if relu else v
    out.backward(_t64(dy))
    r = dict(out=out.detach().numpy(), dx=xt.grad.numpy(), dw=wt.grad.numpy(), dscale=sc.grad.numpy(),
             dshift=sh.grad.numpy(), dres=rt.grad.numpy() if rt is not None else None)
    if bn is not None:      # the chain from (dscale, dshift) through the fold
        torch.autograd.backward([sc_fold, sh_fold], [sc.grad, sh.grad])
        r.update(dbn_weight=bw.grad.numpy(), dbn_bias=bb.grad.numpy())
    return r
