"""The reference of the backbone's stem (is_stem, instance_stixels_core.h f20), independent of the kernel and built on
tests/conv3x3_reference.py and tests/conv_bn_reference.py: the table indexed by the image's bytes, then
torch.nn.functional.conv2d on the CPU in float64 of the half-rounded operands (7x7 with padding 3: `mid`; 3x3 with
padding 1 on A GIVEN `mid`: `out`), the same convolutions of the absolute values, and cb.epilogue64.  The GPU tests
compare `mid` against the reference from the bytes, and `out` against the reference evaluated on the DEVICE'S OWN mid
read back, as f19's block tests do with the device's previous output: a one-ulp flip of an intermediate half is then
not charged to the second layer.

Tolerance.  The fp32 value v the device forms in front of its last rounding is within cb.tolerance of the float64
reference r (147 terms for mid, 144 for out): tol = |scale| terms 2^-23 sum|w x| + ulp_fp32(pre).  The device stores
h = RNE_half(v), and |h - v| <= ulp_half(v) / 2, where ulp_half(v) is the spacing of the half format in v's binade
(2^(e - 10) for float16 with e >= -14, 2^(e - 7) for bfloat16 with e >= -126; the formats' subnormals have the spacing
of their smallest binade).  v is not known to the test, but |v| <= |r| + tol and the spacing does not decrease with
the magnitude, so
    |h - r| <= |h - v| + |v - r| <= ulp_half(|r| + tol) / 2 + tol =: tol_half.
(A value that rounds across a binade boundary is covered: the boundary itself is representable, so the error of
rounding to nearest is at most half the spacing BELOW it, which is smaller.)  The limit on err / tol_half is 1.

Results are cached per case and handed out read-only."""
import functools
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

import conv3x3_reference as cr
import conv_bn_reference as cb

DTYPES = cr.DTYPES
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_FILE = os.path.join(ROOT, "instance_stixels_amd", "csrc", "is_k_stem.hip")

# Normalize's constants of the reference (tools/CNN_training/inference.py:109-110)
MEAN = (0.290101, 0.328081, 0.286964)
STD = (0.182954, 0.186566, 0.184475)
TERMS_MID, TERMS_OUT = 3 * 7 * 7, 16 * 3 * 3


def tile_extents():
    """(rows, cols) of the output tile of a workgroup, from the kernel file's constants."""
    text = open(KERNEL_FILE).read()
    return tuple(int(re.search(r"#define %s (\d+)\b" % name, text).group(1)) for name in ("ST_ROWS", "ST_COLS"))


TILE_ROWS, TILE_COLS = tile_extents()

# (n, rows, cols)
SHAPES = [
    (1, 1, 1),                    # the smallest image
    (2, 3, 3),                    # smaller than either halo; a batch
    (1, 7, 5),                    # smaller than a tile
    (1, 16, 64),                  # a round extent ...
    (1, 17, 65),                  # ... and one row and column more
    (3, 33, 130),                 # ragged tiles both ways; frame independence
]
for _shape in ((1, TILE_ROWS, TILE_COLS), (1, TILE_ROWS + 1, TILE_COLS + 1)):   # exactly one tile, and one more row / column
    if _shape not in SHAPES:
        SHAPES.append(_shape)
SHAPE_IDS = ["%dx%dx%d" % s for s in SHAPES]
WRONG_FORMS_SHAPE = SHAPES.index((1, 7, 5))


def input_table(dtype, mean=MEAN, std=STD):
    """The formula of cnn.input_table written out: fp32 on the CPU, then the cast; float32 numpy [3][256] of values
    that the half dtype holds."""
    unit = torch.arange(256, dtype=torch.float32) / 255
    rows = [((unit - torch.tensor(m, dtype=torch.float32)) / torch.tensor(s, dtype=torch.float32)) for m, s in zip(mean, std)]
    return torch.stack(rows).to(DTYPES[dtype]).float().numpy()


def _operand(a, dtype):
    return torch.from_numpy(np.array(a, np.float64)) if dtype is None else cr.round_half(a, dtype)


def lookup(image, lut64):
    """x[n][c][y][x] = lut[c][image[n][y][x][c]] as a float64 tensor; image uint8 [n][rows][cols][3]."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 4 and image.shape[3] == 3
    lut64 = np.asarray(lut64, np.float64)
    planes = [lut64[c][image[..., c]] for c in range(3)]
    return torch.from_numpy(np.stack(planes, axis=1))


def ulp_half(v, dtype):
    """The spacing of the half format in the binade of |v| (float64 array in, float64 out)."""
    mant, emin = {"float16": (10, -14), "bfloat16": (7, -126)}[dtype]
    v = np.abs(np.asarray(v, np.float64))
    e = np.frexp(v)[1].astype(np.int64) - 1
    e = np.where(v == 0, emin, np.maximum(e, emin))
    return np.ldexp(1.0, (e - mant).astype(np.int64))


def _layer(x64, w, scale, shift, padding, terms, dtype):
    a = F.conv2d(x64, _operand(w, dtype), padding=padding)
    A = F.conv2d(x64.abs(), _operand(w, dtype).abs(), padding=padding)
    pre, _, ref = cb.epilogue64(a, scale, shift, None, True)
    tol = cb.tolerance(pre, pre, A, scale, terms, False)
    r = dict(ref=ref.numpy(), pre=pre.numpy(), A=A.numpy(), tol=tol)
    if dtype is not None:
        r["tol_half"] = tol + 0.5 * ulp_half(np.abs(r["ref"]) + tol, dtype)
    return r


def mid_reference(image, lut, w0, scale0, shift0, dtype):
    """layer0 from the bytes.  dict(ref, pre, A, tol[, tol_half]): `ref` the float64 value in front of the rounding
    to half, tol its bound against the device's fp32 value, tol_half against the device's half (the module's
    docstring).  dtype None: unrounded operands, no tol_half."""
    return _layer(lookup(image, _operand(lut, dtype).numpy()), w0, scale0, shift0, 3, TERMS_MID, dtype)


def out_reference(mid, w1, scale1, shift1, dtype):
    """layer1 on a GIVEN mid [n][16][rows][cols] (values that the half dtype holds; float64 with dtype None)."""
    return _layer(torch.from_numpy(np.array(mid, np.float64)), w1, scale1, shift1, 1, TERMS_OUT, dtype)


def round_mid(r, dtype):
    """The reference's own mid as layer1's operand: ref rounded to the half dtype to nearest even, float64 numpy."""
    return torch.from_numpy(r["ref"]).to(torch.float32).to(DTYPES[dtype]).to(torch.float64).numpy()


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def exact_inputs(s):
    """Inputs whose arithmetic is exact in both dtypes and in any summation order: table values in {0, 1};
    w0 = m (1 + 2^-13) with m in {-1, 0, 1}, which rounds to m; scale0 in {-1, 1}; integer shift0 in [-4, 4]: every
    mid value is an integer of magnitude at most 147 + 4 = 151 < 256.  w1 = (m / 256)(1 + 2^-13) with integer
    |m| <= 255; scale1 in {+-1/2, +-1, +-2}; integer shift1 in [-4, 4]: |a1| <= 144 * 151 * 255 / 256 < 2^15 in
    multiples of 2^-8, exact in fp32, and so is the scaled and shifted value (a multiple of 2^-9 below 2^14, or of 2^-8
    below 2^15 + 4, or of 2^-7 below 2^16 + 4: at most 24 bits)."""
    n, H, W = SHAPES[s]
    rng = np.random.default_rng(5000 + s)
    image = rng.integers(0, 256, (n, H, W, 3)).astype(np.uint8)
    lut = rng.integers(0, 2, (3, 256)).astype(np.float32)
    m0 = rng.integers(-1, 2, (16, 3, 7, 7)).astype(np.float64)
    w0 = (m0 * (1.0 + 2.0 ** -13)).astype(np.float32)
    scale0 = rng.choice(np.array([-1.0, 1.0], np.float32), 16)
    shift0 = rng.integers(-4, 5, 16).astype(np.float32)
    m1 = rng.integers(-255, 256, (16, 16, 3, 3)).astype(np.float64)
    w1 = (m1 / 256.0 * (1.0 + 2.0 ** -13)).astype(np.float32)
    scale1 = rng.choice(np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], np.float32), 16)
    shift1 = rng.integers(-4, 5, 16).astype(np.float32)
    return _frozen(dict(image=image, lut=lut, w0=w0, m0=m0, scale0=scale0, shift0=shift0, w1=w1, m1=m1, scale1=scale1,
                        shift1=shift1))


@functools.lru_cache(maxsize=None)
def exact_reference(s):
    """dict(mid, out) of float64 arrays, every value a half value of both dtypes' (tests/test_stem_cpu.py checks
    that): the same for both dtypes."""
    c = exact_inputs(s)
    mid = _layer(lookup(c["image"], c["lut"]), c["m0"], c["scale0"], c["shift0"], 3, TERMS_MID, None)
    out = _layer(torch.from_numpy(mid["ref"].copy()), c["m1"] / 256.0, c["scale1"], c["shift1"], 1, TERMS_OUT, None)
    return _frozen(dict(mid=mid["ref"], out=out["ref"], a1_abs=out["A"]))


@functools.lru_cache(maxsize=None)
def random_inputs(s):
    """Bytes uniform in 0..255; weights N(0, sqrt(2 / (taps * 16))) (the reference's init, drn.py:191-194); scales in
    +-[0.5, 2]; shift0 uniform in [-1, 1], redrawn until at least a quarter of its channels are above 0.25 (otherwise a
    computed-instead-of-zero mid halo hides behind the ReLU); shift1 N(0, 0.1).  The table is input_table(dtype) of the
    reference's mean and std: lut[c][0] is about -1.6 to -1.8, far from 0."""
    n, H, W = SHAPES[s]
    rng = np.random.default_rng(6000 + s)
    image = rng.integers(0, 256, (n, H, W, 3)).astype(np.uint8)
    w0 = (rng.standard_normal((16, 3, 7, 7)) * np.sqrt(2.0 / (49 * 16))).astype(np.float32)
    w1 = (rng.standard_normal((16, 16, 3, 3)) * np.sqrt(2.0 / (9 * 16))).astype(np.float32)
    scale0 = (rng.uniform(0.5, 2.0, 16) * rng.choice([-1.0, 1.0], 16)).astype(np.float32)
    scale1 = (rng.uniform(0.5, 2.0, 16) * rng.choice([-1.0, 1.0], 16)).astype(np.float32)
    shift0 = rng.uniform(-1.0, 1.0, 16).astype(np.float32)
    while (shift0 > 0.25).sum() < 4:
        shift0 = rng.uniform(-1.0, 1.0, 16).astype(np.float32)
    shift1 = (rng.standard_normal(16) * 0.1).astype(np.float32)
    return _frozen(dict(image=image, w0=w0, scale0=scale0, shift0=shift0, w1=w1, scale1=scale1, shift1=shift1))


@functools.lru_cache(maxsize=None)
def random_mid_reference(s, dtype):
    c = random_inputs(s)
    return _frozen(mid_reference(c["image"], input_table(dtype), c["w0"], c["scale0"], c["shift0"], dtype))


@functools.lru_cache(maxsize=None)
def random_out_reference(s, dtype):
    """layer1 on the REFERENCE's own rounded mid (the CPU tests; the GPU tests take the device's mid)."""
    c = random_inputs(s)
    return _frozen(out_reference(round_mid(random_mid_reference(s, dtype), dtype), c["w1"], c["scale1"], c["shift1"], dtype))


def stem_layers(seed=0, layer1_convs=1):
    """layer0 and layer1 as the reference builds them for arch D (drn.py:154-162 and _make_conv_layers, :223-233),
    written from their description, with statistics as after training; in eval mode."""
    g = torch.Generator().manual_seed(seed)
    conv0 = torch.nn.Conv2d(3, 16, kernel_size=7, stride=1, padding=3, bias=False)
    mods1 = []
    for i in range(layer1_convs):
        mods1 += [torch.nn.Conv2d(16, 16, kernel_size=3, stride=1, padding=1, bias=False, dilation=1),
                  cb.batchnorm(16, seed + 2 + i), torch.nn.ReLU(inplace=True)]
    with torch.no_grad():
        conv0.weight.copy_(torch.randn(conv0.weight.shape, generator=g) * (2.0 / (49 * 16)) ** 0.5)
        for m in mods1[::3]:
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / (9 * 16)) ** 0.5)
    layer0 = torch.nn.Sequential(conv0, cb.batchnorm(16, seed + 1), torch.nn.ReLU(inplace=True))
    return layer0.eval(), torch.nn.Sequential(*mods1).eval()
