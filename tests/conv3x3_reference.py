"""The reference of the backbone tail (is_conv3x3_bn_relu, instance_stixels_core.h f17), independent of the kernel:
torch.nn.functional.conv2d on the CPU in float64 of the half-rounded operands with padding = dilation -- the module the
reference's drn.py is made of -- the same convolution of the absolute values (A = sum |w x|, what the error bound
scales with), and the epilogue in float64.  Results are cached per case and handed out read-only."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16}

# (n, channels_in, channels_out, rows8, cols8, dilation)
SHAPES = [
    (2, 16, 32, 5, 7, 1),         # one k-step, the image inside one tile, an odd width
    (1, 48, 64, 9, 37, 2),        # two output tiles, a ragged column tile
    (3, 32, 32, 3, 70, 4),        # dilation >= rows8: the top and bottom tap rows wholly outside
    (1, 16, 32, 1, 1, 8),         # only the centre tap lands
    (1, 512, 512, 16, 32, 2),     # the real channel counts
    (1, 64, 64, 128, 256, 1),     # the real plane
]
SHAPE_IDS = ["%dx%d-%dx%dx%d-d%d" % s for s in SHAPES]


def round_half(a, dtype):
    """fp32 values rounded to the half dtype (round to nearest even, torch's conversion on the CPU), as a float64
    tensor."""
    return torch.tensor(np.asarray(a, np.float32)).to(DTYPES[dtype]).to(torch.float64)


def conv64(x64, w64, dilation):
    """(a, A): the convolution of float64 operands and that of their absolute values, padding = dilation."""
    a = F.conv2d(x64, w64, padding=dilation, dilation=dilation)
    A = F.conv2d(x64.abs(), w64.abs(), padding=dilation, dilation=dilation)
    return a, A


def epilogue64(a, scale, shift, relu):
    """scale[co] * a + shift[co], then max(v, 0) with relu, in float64 (scale, shift: fp32 arrays)."""
    sc = torch.from_numpy(np.asarray(scale, np.float64)).view(1, -1, 1, 1)
    sh = torch.from_numpy(np.asarray(shift, np.float64)).view(1, -1, 1, 1)
    v = sc * a + sh
    return torch.clamp_min(v, 0.0) if relu else v


def tolerance(ref, A, scale, channels_in):
    """|scale| * 9 channels_in * 2^-23 * A + ulp_fp32(ref): the n = 9 channels_in exact products summed in any
    order, each addition off by at most 2^-23 relative, stay within n 2^-23 A of their sum (round to nearest in any
    order with a factor 2 to spare; chopping too); the fmaf adds one rounding; ReLU is 1-Lipschitz."""
    sc = torch.from_numpy(np.abs(np.asarray(scale, np.float64))).view(1, -1, 1, 1)
    ulp = np.spacing(np.abs(ref.numpy()).astype(np.float32)).astype(np.float64)
    return (sc * (9 * channels_in * 2.0 ** -23) * A).numpy() + ulp


def reference(x, w, scale, shift, dilation, dtype, relu=True):
    """fp32 arrays in; dict(ref, A, tol) of float64 arrays for the operands rounded to `dtype`."""
    a, A = conv64(round_half(x, dtype), round_half(w, dtype), dilation)
    ref = epilogue64(a, scale, shift, relu)
    return dict(ref=ref.numpy(), A=A.numpy(), tol=tolerance(ref, A, scale, x.shape[1]))


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def exact_inputs(s):
    """Inputs whose arithmetic is exact in every order: features integers in {0..3}, weights (m / 256)(1 + 2^-13) with
    integer |m| <= 255 (exact in fp32: 8 + 13 bits; the pack call must round them back to m / 256 in either half
    dtype), scale 1, shift 0.  Products are multiples of 2^-8, and at channels_in = 512 every partial sum is below
    9 * 512 * 3 < 2^14: exact in fp32."""
    n, cin, cout, H, W, d = SHAPES[s]
    rng = np.random.default_rng(1000 + s)
    x = rng.integers(0, 4, (n, cin, H, W)).astype(np.float32)
    m = rng.integers(-255, 256, (cout, cin, 3, 3)).astype(np.float64)
    w = (m / 256.0 * (1.0 + 2.0 ** -13)).astype(np.float32)
    return _frozen(dict(x=x, w=w, m=m, scale=np.ones(cout, np.float32), shift=np.zeros(cout, np.float32)))


@functools.lru_cache(maxsize=None)
def exact_reference(s, relu=True):
    """The float64 reference of exact_inputs(s); the same for both half dtypes, which hold these operands exactly
    (tests/test_conv3x3_cpu.py checks that)."""
    c = exact_inputs(s)
    x64 = torch.from_numpy(c["x"].astype(np.float64))
    w64 = torch.from_numpy(c["m"] / 256.0)
    a, A = conv64(x64, w64, SHAPES[s][5])
    return _frozen(dict(ref=epilogue64(a, c["scale"], c["shift"], relu).numpy(), A=A.numpy()))


@functools.lru_cache(maxsize=None)
def random_inputs(s):
    """The issue's random inputs: features |N(0, 1)|, weights N(0, sqrt(2 / (9 channels_out))) (the reference's init,
    drn.py:191-194), scale in +-[0.5, 2], shift N(0, 0.1); fp32."""
    n, cin, cout, H, W, d = SHAPES[s]
    rng = np.random.default_rng(2000 + s)
    x = np.abs(rng.standard_normal((n, cin, H, W))).astype(np.float32)
    w = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cout))).astype(np.float32)
    scale = (rng.uniform(0.5, 2.0, cout) * rng.choice([-1.0, 1.0], cout)).astype(np.float32)
    shift = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    return _frozen(dict(x=x, w=w, scale=scale, shift=shift))


@functools.lru_cache(maxsize=None)
def random_reference(s, dtype, relu=True):
    c = random_inputs(s)
    return _frozen(reference(c["x"], c["w"], c["scale"], c["shift"], SHAPES[s][5], dtype, relu))
