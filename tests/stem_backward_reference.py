"""The reference of the backward pass of the stem (is_stem_backward, instance_stixels_core.h f23), independent of the
kernel and built on tests/stem_reference.py and tests/conv_backward_reference.py: the masked gradients by torch's CPU
conversion on the rounded operands; dMid, G1 and G0 by torch float64 on the CPU (torch.nn.grad.conv2d_input /
conv2d_weight) of the half-rounded operands as the contract names them, including round_half(scale1 * w1_half); the
same contractions of the absolute values, which the bounds scale with.  Everything behind a gh takes that gh as an
argument: the GPU tests pin gh1 bit for bit, dMid and the gradients of layer1 on the device's own gh1, and the gradients
of layer0 on the device's own gh0, so a one-ulp flip of an intermediate half is not charged to the next stage.

Bounds, in the form of conv_backward_reference.backward:
  dMid    144 2^-23 sum|wT1 gh1| + ulp_fp32(dMid) for the fp32 value in front of the rounding, plus the half ulp of the
          rounding (stem_reference's tol_half form).
  G       (terms_chunk 2^-23 + chunks 2^-53) sum|gh x|: a chunk's accumulator adds at most terms_chunk exact products,
          terms_chunk = the chunk's rows times its columns rounded up to whole K steps of 32; the binary64 sum of the
          chunks' partials adds chunks 2^-53.
  dW      |scale| tol_G + ulp_fp32(dW);  dscale  sum |w_half| tol_G + (channels_in taps) 2^-53 sum|w_half G| +
          ulp_fp32(dscale);  dshift  (n P) 2^-53 sum|gh| + ulp_fp32(dshift): f21's expressions.
The limit on err / tol is 1.

Results are cached per case and handed out read-only."""
import functools
import os
import re

import numpy as np
import torch
import torch.nn.grad as G

import conv3x3_reference as cr
import conv_backward_reference as cbr
import conv_stride_backward_reference as csr
import stem_reference as sr

DTYPES = sr.DTYPES
ROOT = sr.ROOT
HEADER = os.path.join(ROOT, "include", "instance_stixels_core.h")


def _header_constant(name):
    return int(re.search(r"#define %s (\d+)\b" % name, open(HEADER).read()).group(1))


BAND = _header_constant("IS_STEM_BACKWARD_BAND")
SEGMENT = _header_constant("IS_STEM_BACKWARD_SEGMENT")
TILE_ROWS = _header_constant("IS_STEM_BACKWARD_TILE_ROWS")
TILE_COLS = _header_constant("IS_STEM_BACKWARD_TILE_COLS")

# (n, rows, cols): the forward's shapes and the backward tile's own extents, two and three bands, two segments, and the
# batch of source (b)
SHAPES = list(sr.SHAPES)
for _shape in ((1, TILE_ROWS, TILE_COLS), (1, TILE_ROWS + 1, TILE_COLS + 1), (1, BAND + 1, 9), (2, 2 * BAND + 3, 5),
               (1, 3, SEGMENT + 1), (2, 33, 130)):
    if _shape not in SHAPES:
        SHAPES.append(_shape)
SHAPE_IDS = ["%dx%dx%d" % s for s in SHAPES]
WRONG_FORMS_SHAPE = SHAPES.index((1, 7, 5))

# source (b), the gradient from layer2's masked gradient: (index into SHAPES, channels_next)
NEXT_CASES = [(SHAPES.index((1, 7, 5)), 32), (SHAPES.index((1, 16, 64)), 32), (SHAPES.index((1, 17, 65)), 32),
              (SHAPES.index((2, 33, 130)), 32), (SHAPES.index((1, 17, 65)), 64)]
NEXT_IDS = ["%s-c%d" % (SHAPE_IDS[s], cn) for s, cn in NEXT_CASES]

_t64 = cbr._t64
_ulp32 = cbr._ulp32


def chunks_of(n, H, W):
    return n * ((H + BAND - 1) // BAND) * ((W + SEGMENT - 1) // SEGMENT)


def terms_chunk(H, W):
    """The products of the largest chunk's accumulator: its rows times its columns rounded up to whole K steps of 32."""
    return min(BAND, H) * ((min(SEGMENT, W) + 31) // 32 * 32)


def masked_gradient(dy, stored, dtype):
    """round_half(dy) where the stored tensor is > 0, else +0, as a tensor of the half dtype."""
    return cbr.masked_gradient(dy, stored, True, dtype)


def next_gradient(gh_next, w_next, scale_next, shape, dtype):
    """g_out [n][16][H][W] (shape) from the masked gradient of the stride-2 3x3 layer that reads `out`: f22's dX formula,
    by conv_stride_backward_reference's torch.nn.grad.conv2d_input at stride 2 on round_half(scale_next * w_next_half).
    dict(ref, tol, tol_half) as data_gradient; terms = 4 * channels_next."""
    g64 = gh_next.double() if torch.is_tensor(gh_next) else _t64(gh_next)
    ws = cbr.scaled_weight(w_next, scale_next, dtype)
    kw = dict(stride=2, padding=1)
    ref = G.conv2d_input(tuple(shape), ws, g64, **kw)
    A = G.conv2d_input(tuple(shape), ws.abs(), g64.abs(), **kw)
    assert (csr.taps_of_class(shape[2], shape[3], 3) <= 4).all()
    tol = (4 * ws.shape[0] * 2.0 ** -23) * A.numpy() + _ulp32(ref.numpy())
    return dict(ref=ref.numpy(), tol=tol, tol_half=tol + 0.5 * sr.ulp_half(np.abs(ref.numpy()) + tol, dtype))


def data_gradient(gh1, w1, scale1, dtype, flip=True):
    """dMid from a given gh1 (a half tensor or an array of its values).  dict(ref, tol, tol_half): the float64 value in
    front of the rounding to half, its bound against the device's fp32 value and against the device's half.  flip =
    False is the wrong form without the tap flip (the CPU tests)."""
    g64 = gh1.double() if torch.is_tensor(gh1) else _t64(gh1)
    ws = cbr.scaled_weight(w1, scale1, dtype)
    if not flip:
        ws = ws.flip(2, 3)
    ref = G.conv2d_input(g64.shape, ws, g64, padding=1)
    A = G.conv2d_input(g64.shape, ws.abs(), g64.abs(), padding=1)
    tol = (sr.TERMS_OUT * 2.0 ** -23) * A.numpy() + _ulp32(ref.numpy())
    return dict(ref=ref.numpy(), tol=tol, tol_half=tol + 0.5 * sr.ulp_half(np.abs(ref.numpy()) + tol, dtype))


def weight_gradients(x64, w, scale, gh, padding, dtype):
    """G, dW, dscale and dshift of one layer from its operand x64 (a float64 tensor of half values, [n][ci][H][W]), its
    fp32 master weight and folded scale and a given gh, with their bounds: dict(G, dw, dscale, dshift, tol_G, tol_dw,
    tol_dscale, tol_dshift) of float64 arrays."""
    g64 = gh.double() if torch.is_tensor(gh) else _t64(gh)
    wh64 = cr.round_half(w, dtype) if dtype is not None else _t64(w)
    n, cin, H, W = x64.shape
    taps = wh64.shape[2] * wh64.shape[3]
    sc = _t64(scale)
    Gsum = G.conv2d_weight(x64, wh64.shape, g64, padding=padding)
    Gabs = G.conv2d_weight(x64.abs(), wh64.shape, g64.abs(), padding=padding)
    tol_G = (terms_chunk(H, W) * 2.0 ** -23 + chunks_of(n, H, W) * 2.0 ** -53) * Gabs
    dw = sc.view(-1, 1, 1, 1) * Gsum
    dscale = (wh64 * Gsum).sum((1, 2, 3))
    dshift = g64.sum((0, 2, 3))
    return dict(
        G=Gsum.numpy(), dw=dw.numpy(), dscale=dscale.numpy(), dshift=dshift.numpy(), tol_G=tol_G.numpy(),
        tol_dw=(sc.abs().view(-1, 1, 1, 1) * tol_G).numpy() + _ulp32(dw.numpy()),
        tol_dscale=((wh64.abs() * tol_G).sum((1, 2, 3)) + cin * taps * 2.0 ** -53 * (wh64 * Gsum).abs().sum((1, 2, 3))).numpy()
        + _ulp32(dscale.numpy()),
        tol_dshift=(n * H * W * 2.0 ** -53 * g64.abs().sum((0, 2, 3))).numpy() + _ulp32(dshift.numpy()))


def layer1_gradients(mid, w1, scale1, gh1, dtype):
    """The gradients of layer1's parameters from the STORED mid (half values) and a given gh1."""
    return weight_gradients(_t64(mid), w1, scale1, gh1, 1, dtype)


def layer0_operand(image, lut, dtype, pad_with_table=False):
    """x of layer0 as a float64 tensor.  pad_with_table: the wrong form whose padding is lut[c][0] instead of nothing,
    returned with the padding in place ([n][3][H + 6][W + 6]; convolve it with padding 0)."""
    lut64 = sr._operand(lut, dtype).numpy()
    x = sr.lookup(image, lut64)
    if not pad_with_table:
        return x
    n, _, H, W = x.shape
    padded = torch.from_numpy(np.broadcast_to(lut64[:, 0].reshape(1, 3, 1, 1), (n, 3, H + 6, W + 6)).copy())
    padded[:, :, 3:3 + H, 3:3 + W] = x
    return padded


def layer0_gradients(image, lut, w0, scale0, gh0, dtype):
    """The gradients of layer0's parameters from the image's bytes, the table and a given gh0."""
    return weight_gradients(layer0_operand(image, lut, dtype), w0, scale0, gh0, 3, dtype)


def forward_halves(c, lut, dtype):
    """(mid, out) of the reference's own forward as float32 arrays of half values: stem_reference's layers, each rounded
    to the half dtype to nearest even."""
    m = sr.mid_reference(c["image"], lut, c["w0"], c["scale0"], c["shift0"], dtype)
    mid = sr.round_mid(m, dtype)
    o = sr.out_reference(mid, c["w1"], c["scale1"], c["shift1"], dtype)
    return mid.astype(np.float32), sr.round_mid(o, dtype).astype(np.float32)


def chain(c, lut, mid, out, dtype):
    """The whole backward on the reference's own intermediates (the CPU tests and the exact family): dict(gh1, gh0 (half
    tensors), dmid, l1, l0)."""
    gh1 = masked_gradient(c["dy"], out, dtype)
    dmid = data_gradient(gh1, c["w1"], c["scale1"], dtype)
    gh0 = masked_gradient(dmid["ref"].astype(np.float32), mid, dtype)
    return dict(gh1=gh1, gh0=gh0, dmid=dmid, l1=layer1_gradients(mid, c["w1"], c["scale1"], gh1, dtype),
                l0=layer0_gradients(c["image"], lut, c["w0"], c["scale0"], gh0, dtype))


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def random_inputs(s):
    """stem_reference.random_inputs' family at this file's shapes, with dY N(0, 1)."""
    n, H, W = SHAPES[s]
    rng = np.random.default_rng(7000 + s)
    image = rng.integers(0, 256, (n, H, W, 3)).astype(np.uint8)
    w0 = (rng.standard_normal((16, 3, 7, 7)) * np.sqrt(2.0 / (49 * 16))).astype(np.float32)
    w1 = (rng.standard_normal((16, 16, 3, 3)) * np.sqrt(2.0 / (9 * 16))).astype(np.float32)
    scale0 = (rng.uniform(0.5, 2.0, 16) * rng.choice([-1.0, 1.0], 16)).astype(np.float32)
    scale1 = (rng.uniform(0.5, 2.0, 16) * rng.choice([-1.0, 1.0], 16)).astype(np.float32)
    shift0 = rng.uniform(-1.0, 1.0, 16).astype(np.float32)
    shift1 = (rng.standard_normal(16) * 0.1).astype(np.float32)
    dy = rng.standard_normal((n, 16, H, W)).astype(np.float32)
    return _frozen(dict(image=image, w0=w0, scale0=scale0, shift0=shift0, w1=w1, scale1=scale1, shift1=shift1, dy=dy))


@functools.lru_cache(maxsize=None)
def exact_inputs(s):
    """stem_reference.exact_inputs' family with smaller magnitudes behind layer0, at this file's shapes: table values in
    {0, 1}; w0 = m (1 + 2^-13) with m in {-1, 0, 1}; scale0 in {-1, 1}; integer shift0 in [-4, 4]: mid is an integer of
    at most 151.  w1 = m (1 + 2^-13) with m in {-1, 0, 1}, three quarters of them 0; scale1 in {-1, 1}; integer shift1
    in [-4, 4]; dY in {-1, 0, 1}.  Then wT1 is in {-1, 0, 1}, dMid an integer of at most 144 (a value of both half
    dtypes), gh1 mid an integer of at most 151 and gh0 x one of at most 144: a chunk adds at most BAND * SEGMENT of them,
    below 2^24.  tests/test_stem_backward_cpu.py proves both per shape from the absolute-value contractions."""
    n, H, W = SHAPES[s]
    rng = np.random.default_rng(8000 + s)
    image = rng.integers(0, 256, (n, H, W, 3)).astype(np.uint8)
    lut = rng.integers(0, 2, (3, 256)).astype(np.float32)
    m0 = rng.integers(-1, 2, (16, 3, 7, 7)).astype(np.float64)
    m1 = (rng.integers(-1, 2, (16, 16, 3, 3)) * (rng.integers(0, 4, (16, 16, 3, 3)) == 0)).astype(np.float64)
    w0 = (m0 * (1.0 + 2.0 ** -13)).astype(np.float32)
    w1 = (m1 * (1.0 + 2.0 ** -13)).astype(np.float32)
    scale0 = rng.choice(np.array([-1.0, 1.0], np.float32), 16)
    scale1 = rng.choice(np.array([-1.0, 1.0], np.float32), 16)
    shift0 = rng.integers(-4, 5, 16).astype(np.float32)
    shift1 = rng.integers(-4, 5, 16).astype(np.float32)
    dy = rng.integers(-1, 2, (n, 16, H, W)).astype(np.float32)
    return _frozen(dict(image=image, lut=lut, w0=w0, m0=m0, scale0=scale0, shift0=shift0, w1=w1, m1=m1, scale1=scale1,
                        shift1=shift1, dy=dy))


def _exact_chain(c, dy):
    mid = sr._layer(sr.lookup(c["image"], c["lut"]), c["m0"], c["scale0"], c["shift0"], 3, sr.TERMS_MID, None)["ref"]
    out = sr._layer(_t64(mid), c["m1"], c["scale1"], c["shift1"], 1, sr.TERMS_OUT, None)["ref"]
    gh1 = np.where(out > 0, np.asarray(dy, np.float64), 0.0)
    wT = _t64(c["scale1"]).view(-1, 1, 1, 1) * _t64(c["m1"])
    dmid = G.conv2d_input(gh1.shape, wT, _t64(gh1), padding=1).numpy()
    gh0 = np.where(mid > 0, dmid, 0.0)
    l1 = weight_gradients(_t64(mid), c["m1"], c["scale1"], gh1, 1, None)
    l0 = weight_gradients(sr.lookup(c["image"], c["lut"]), c["m0"], c["scale0"], gh0, 3, None)
    return _frozen(dict(mid=mid, out=out, gout=np.asarray(dy, np.float64), gh1=gh1, dmid=dmid, gh0=gh0, dw0=l0["dw"],
                        dscale0=l0["dscale"], dshift0=l0["dshift"], dw1=l1["dw"], dscale1=l1["dscale"],
                        dshift1=l1["dshift"]))


@functools.lru_cache(maxsize=None)
def exact_reference(s):
    """The exact family in float64 on the integer weights m0 and m1, no rounding anywhere: dict(mid, out (the values in
    front of the forward's rounding to half), gout, gh1, dmid, gh0, dw0, dscale0, dshift0, dw1, dscale1, dshift1).  mid,
    gh1, dmid and gh0 are values of both half dtypes; the fp32 outputs are the float64 values rounded once."""
    c = exact_inputs(s)
    return _exact_chain(c, c["dy"])


@functools.lru_cache(maxsize=None)
def exact_reference_next(s, cn):
    """exact_reference with source (b): g_out from next_inputs(s, cn, "exact") on its integer weights."""
    c, nx = exact_inputs(s), next_inputs(s, cn, "exact")
    wT = _t64(nx["scale"]).view(-1, 1, 1, 1) * _t64(nx["m"])
    gout = G.conv2d_input(c["dy"].shape, wT, _t64(nx["gh"]), stride=2, padding=1).numpy()
    return _exact_chain(c, gout)


@functools.lru_cache(maxsize=None)
def next_inputs(s, cn, kind):
    """layer2's side of source (b) for shape s: weight [cn][16][3][3], scale [cn] and the
    masked gradient gh [n][cn][ceil(H / 2)][ceil(W / 2)], about half of it zero.  random: N(0, sqrt(2 / (9 cn))) weights,
    scales in +-[0.5, 2], gh N(0, 1).  exact: weights in {-1, 0, 1} (1 + 2^-13), seven eighths of them 0, scales +-1, gh
    in {-1, 0, 1}: g_out is an integer of at most 4 cn / 8 on average and never above 4 cn <= 512, whose half rounding
    tests/test_stem_backward_cpu.py checks to be exact."""
    n, H, W = SHAPES[s]
    rng = np.random.default_rng(9000 + 10 * s + cn + (0 if kind == "random" else 1))
    shape = (n, cn, (H + 1) // 2, (W + 1) // 2)
    active = rng.integers(0, 2, shape)
    if kind == "random":
        w = (rng.standard_normal((cn, 16, 3, 3)) * np.sqrt(2.0 / (9 * cn))).astype(np.float32)
        scale = (rng.uniform(0.5, 2.0, cn) * rng.choice([-1.0, 1.0], cn)).astype(np.float32)
        gh = (rng.standard_normal(shape) * active).astype(np.float32)
        return _frozen(dict(w=w, scale=scale, gh=gh))
    m = (rng.integers(-1, 2, (cn, 16, 3, 3)) * (rng.integers(0, 8, (cn, 16, 3, 3)) == 0)).astype(np.float64)
    scale = rng.choice(np.array([-1.0, 1.0], np.float32), cn)
    gh = (rng.integers(-1, 2, shape) * active).astype(np.float32)
    return _frozen(dict(w=(m * (1.0 + 2.0 ** -13)).astype(np.float32), m=m, scale=scale, gh=gh))


def autograd64(c, lut64):
    """float64 torch.autograd of relu(bn1(conv(relu(bn0(conv(x)))))) against dY on the operands as given (unrounded):
    dict(mid, out, dw0, dscale0, dshift0, dw1, dscale1, dshift1)."""
    leaf = lambda a: _t64(a).requires_grad_(True)
    x = sr.lookup(c["image"], lut64)
    p = {k: leaf(c[k]) for k in ("w0", "scale0", "shift0", "w1", "scale1", "shift1")}
    conv = torch.nn.functional.conv2d
    mid = torch.relu(p["scale0"].view(1, -1, 1, 1) * conv(x, p["w0"], padding=3) + p["shift0"].view(1, -1, 1, 1))
    out = torch.relu(p["scale1"].view(1, -1, 1, 1) * conv(mid, p["w1"], padding=1) + p["shift1"].view(1, -1, 1, 1))
    out.backward(_t64(c["dy"]))
    r = {"d" + k: v.grad.numpy() for k, v in p.items()}
    r.update(mid=mid.detach().numpy(), out=out.detach().numpy())
    return r
