"""The backbone's stem (f20) without a GPU: the symbols, bindings and contract text, the struct layout against a
compiled probe, the refusals of is_stem (all made before the device is touched), is_stem_packed_bytes,
cnn.input_table against its formula per byte, the reference of tests/stem_reference.py pinned against layer0 / layer1
built as the reference builds them, against the claim that its exact inputs are exact and against three wrong forms of
a fused stem that its bound has to catch, the refusals of cnn.DrnStem (made before anything is packed), and the
signatures of the new Python surface."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv3x3_reference as cr
import conv_bn_reference as cb
import stem_reference as sr
from instance_stixels_amd import cnn, core

ROOT = sr.ROOT
HEADER = os.path.join(ROOT, "include", "instance_stixels_core.h")


def test_symbols_are_declared_exported_and_bound():
    header = open(HEADER).read()
    for name in ("is_stem_packed_bytes", "is_stem_pack_weights", "is_stem"):
        assert name + "(" in header and name in core.EXPORTS and hasattr(core.lib(), name), name
    for fn in ("stem_packed_bytes", "stem_pack_weights", "stem_ptr", "stem"):
        assert callable(getattr(core, fn)), fn
    assert issubclass(core.StemArgs, ctypes.Structure)
    assert callable(cnn.input_table) and callable(cnn.DrnStem) and callable(cnn.Drn) and callable(cnn.Drn.from_base)
    # the contract stands in the header and at the top of the kernel file
    kernel = open(sr.KERNEL_FILE).read()
    for text in (header, kernel):
        flat = re.sub(r"\s*\n\s*\*\s*", " ", text)
        assert "drn.py:154-159" in flat and "drn.py:161-162" in flat
        assert "lut[c][ image[n][y][x][c] ]" in flat
        assert re.search(r"zero padding of the NORMALISED value", flat) and "lut[c][0]" in flat
        assert re.search(r"mid pixel (OUTSIDE THE IMAGE IS ZERO|outside the image is ZERO)", flat) and "relu(shift0)" in flat
        assert "x[n][ci][y + ky - 3][x + kx - 3]" in flat and "mid[n][ci][y + ky - 1][x + kx - 1]" in flat
        assert "fmaf(scale0[co], a0, shift0[co])" in flat and "fmaf(scale1[co], a1, shift1[co])" in flat
        assert re.search(r"same bytes whether or not d_mid is given", flat) and "no atomics" in flat
        assert "n_images * rows * cols * 3 bytes" in flat or "n * rows * cols * 3 bytes" in flat
        assert "v_mfma_f32_16x16x32_{f16,bf16}" in flat
    assert "static_assert(ST_LDS_BYTES <= 65536" in kernel
    assert "is_k_stem.hip" in open(os.path.join(ROOT, "instance_stixels_amd", "csrc", "Makefile")).read()
    launch = open(os.path.join(ROOT, "instance_stixels_amd", "csrc", "is_launch.h")).read()
    assert launch.count("isk_launch_stem(") == 1 and launch.count("isk_launch_stem_pack(") == 1


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "instance_stixels_core.h"
#define F(f) printf(#f " %zu %zu\n", offsetof(is_stem_args, f), sizeof(((is_stem_args*)0)->f));
int main() {
    printf(". %zu 0\n", sizeof(is_stem_args));
    FIELDS
    return 0;
}
"""


def test_args_layout_matches_the_header(tmp_path):
    fields = core.StemArgs._fields_
    (tmp_path / "probe.cpp").write_text(PROBE.replace("FIELDS", "".join(f"F({n})" for n, _ in fields)))
    exe = str(tmp_path / "probe")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "probe.cpp"), "-o", exe],
                   check=True)
    got = {f: (int(off), int(size)) for f, off, size in
           (l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())}
    assert got["."][0] == ctypes.sizeof(core.StemArgs) == 112                        # the struct's size is pinned
    declared = re.search(r"typedef struct is_stem_args \{(.*?)\} is_stem_args;", open(HEADER).read(), re.S).group(1)
    declared = re.sub(r"/\*.*?\*/", "", declared, flags=re.S)
    names = re.findall(r"(\w+)(?:\[4\])?\s*[,;]", declared)
    assert names == [n for n, _ in fields]
    assert names == ["d_image", "n_images", "rows", "cols", "d_lut", "dtype", "d_packed", "d_scale0", "d_shift0",
                     "d_scale1", "d_shift1", "d_mid", "d_out", "reserved"]
    for name, _ in fields:
        field = getattr(core.StemArgs, name)
        assert got[name] == (field.offset, field.size), name


# A call that would be accepted (the pointers are never dereferenced on the host: every case below is refused before
# the device is touched).  Image 2 * 5 * 7 * 3 = 210 B at 0x10000; mid and out 2 * 16 * 5 * 7 * 2 = 2240 B each.
GOOD = dict(d_image=0x10000, n_images=2, rows=5, cols=7, d_lut=0x20000, dtype=core.HEAD_BF16, d_packed=0x30000,
            d_scale0=0x40000, d_shift0=0x40100, d_scale1=0x40200, d_shift1=0x40300, d_mid=0x50000, d_out=0x60000)
RESERVED = dict(reserved=(0, 0, 1, 0))


def _refused(call):
    assert core.stem_ptr(**call) == -1                                         # IS_EINVAL
    return core.lib().is_last_error().decode()


@pytest.mark.parametrize("change, message", [
    (dict(d_image=None), "null"), (dict(d_lut=None), "null"), (dict(d_packed=None), "null"),
    (dict(d_scale0=None), "null"), (dict(d_shift0=None), "null"), (dict(d_scale1=None), "null"),
    (dict(d_shift1=None), "null"), (dict(d_out=None), "null"),
    (dict(dtype=core.HEAD_F32), "dtype is neither IS_HEAD_F16 nor IS_HEAD_BF16"),
    (dict(dtype=7), "dtype is neither"), (dict(dtype=-1), "dtype is neither"),
    (dict(n_images=0), "n_images"), (dict(n_images=65536), "n_images"),
    (dict(rows=0), "rows and cols"), (dict(rows=32768), "rows and cols"),
    (dict(cols=0), "rows and cols"), (dict(cols=32768), "rows and cols"), (dict(cols=-3), "rows and cols"),
    (dict(d_packed=0x30008), "d_packed must be 16-byte aligned"),
    (dict(d_lut=0x20001), "d_lut must be aligned"),
    (dict(d_mid=0x50001), "d_mid must be aligned"),
    (dict(d_out=0x60001), "d_out must be aligned"),
    (dict(d_shift1=0x40302), "4-byte aligned"),
    # every buffer at its own size: mid and out are 2240 B, the image 210 B
    (dict(d_out=0x50000 + 2238), "d_out overlaps d_mid"),
    (dict(d_out=0x50000 - 2238), "d_out overlaps d_mid"),
    (dict(d_out=0x50000), "d_out overlaps d_mid"),
    (dict(d_out=0x10000 + 208), "d_out overlaps d_image"),
    (dict(d_out=0x10000 - 2238), "d_out overlaps d_image"),
    (dict(d_mid=0x10000 + 208), "d_mid overlaps d_image"),
    (dict(d_mid=0x10000 - 2238), "d_mid overlaps d_image"),
    (dict(d_mid=None, d_out=0x10000 + 208), "d_out overlaps d_image"),
    (RESERVED, "reserved"),
    (dict(reserved=(-1, 0, 0, 0), d_mid=None), "reserved"),
])
def test_refusals_need_no_device(change, message):
    assert re.search(message, _refused(dict(GOOD, **change)))


def test_calls_refused_for_reserved_alone_have_passed_every_other_check():
    """A call accepted up to the device cannot be run here.  The reserved fields are checked last, so a call refused
    for them alone has passed every other check: both dtypes, no d_mid, the extreme extents, buffers that touch at each
    one's own size."""
    calls = [
        GOOD, dict(GOOD, dtype=core.HEAD_F16), dict(GOOD, d_mid=None),
        dict(GOOD, d_out=0x50000 + 2240), dict(GOOD, d_out=0x50000 - 2240),
        dict(GOOD, d_out=0x10000 + 210), dict(GOOD, d_out=0x10000 - 2240),
        dict(GOOD, d_mid=0x10000 + 210), dict(GOOD, d_mid=0x10000 - 2240),
        dict(GOOD, n_images=1, rows=1, cols=1),
        dict(GOOD, n_images=65535, d_image=0x10000000, d_mid=0x20000000, d_out=0x30000000),
        dict(GOOD, n_images=1, rows=32767, cols=32767, d_image=0x1000, d_mid=None, d_out=0x7f0000000000),
    ]
    for call in calls:
        message = _refused(dict(call, **RESERVED))
        assert "reserved" in message and "overlap" not in message, (call, message)
    assert core.lib().is_stem(None, None) == -1 and b"null args" in core.lib().is_last_error()


def test_packed_bytes_and_the_packers_refusals():
    assert core.stem_packed_bytes(core.HEAD_F16) == core.stem_packed_bytes(core.HEAD_BF16) > 0
    # the blob holds the 16 * 147 + 16 * 144 values (and zeros), in whole 16-byte fragments
    assert core.stem_packed_bytes(core.HEAD_BF16) % 16 == 0 and core.stem_packed_bytes(core.HEAD_BF16) >= 2 * 16 * (147 + 144)
    assert core.stem_packed_bytes(core.HEAD_F32) == 0 and core.stem_packed_bytes(9) == 0
    L = core.lib()
    for args, message in [((None, 0x2000, core.HEAD_BF16, 0x3000), b"null"), ((0x1000, None, core.HEAD_BF16, 0x3000), b"null"),
                          ((0x1000, 0x2000, core.HEAD_BF16, None), b"null"),
                          ((0x1000, 0x2000, core.HEAD_F32, 0x3000), b"dtype"),
                          ((0x1002, 0x2000, core.HEAD_F16, 0x3000), b"4-byte"),
                          ((0x1000, 0x2000, core.HEAD_F16, 0x3008), b"16-byte")]:
        assert L.is_stem_pack_weights(*args, None) == -1 and message in L.is_last_error(), args
    with pytest.raises(core.CoreError, match="neither torch.float16 nor torch.bfloat16"):
        core.stem_pack_weights(np.zeros((16, 3, 7, 7), np.float32), np.zeros((16, 16, 3, 3), np.float32), torch.float32)
    with pytest.raises(core.CoreError, match=r"\[16\]\[3\]\[7\]\[7\]"):
        core.stem_pack_weights(np.zeros((16, 3, 3, 3), np.float32), np.zeros((16, 16, 3, 3), np.float32), torch.float16)


@pytest.mark.parametrize("dtype", sorted(sr.DTYPES))
def test_input_table_is_the_formula_per_byte(dtype):
    td = sr.DTYPES[dtype]
    table = cnn.input_table(sr.MEAN, sr.STD, td)
    assert table.dtype == td and tuple(table.shape) == (3, 256) and table.device.type == "cpu"
    for c in range(3):
        for byte in range(256):
            v = (np.float32(byte) / np.float32(255) - np.float32(sr.MEAN[c])) / np.float32(sr.STD[c])
            assert v.dtype == np.float32
            want = torch.tensor(v).to(td)
            assert table[c, byte].view(torch.int16) == want.view(torch.int16), (c, byte)
    assert np.array_equal(table.float().numpy(), sr.input_table(dtype))
    assert -1.85 < float(table[:, 0].max()) < -1.5                             # lut[c][0] is far from 0
    # ToTensor + Normalize, as torch computes them on an image
    image = torch.arange(256, dtype=torch.uint8).view(1, 16, 16, 1).expand(1, 16, 16, 3)
    x = image.permute(0, 3, 1, 2).float() / 255
    x = ((x - torch.tensor(sr.MEAN).view(1, 3, 1, 1)) / torch.tensor(sr.STD).view(1, 3, 1, 1)).to(td)
    got = sr.lookup(image.numpy(), table.float().numpy())
    assert torch.equal(got, x.double())
    with pytest.raises(core.CoreError, match="float16 nor torch.bfloat16"):
        cnn.input_table(sr.MEAN, sr.STD, torch.float32)
    with pytest.raises(core.CoreError, match="three values"):
        cnn.input_table(sr.MEAN[:2], sr.STD, td)
    assert "import torchvision" not in open(os.path.join(ROOT, "instance_stixels_amd", "cnn.py")).read()


def _fold64(bn):
    scale = (bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)).detach()
    return scale.numpy(), (bn.bias.double() - bn.running_mean.double() * scale).detach().numpy()


@pytest.mark.parametrize("n, rows, cols", [(2, 9, 11), (1, 1, 1), (1, 3, 20)])
def test_reference_is_layer0_and_layer1_of_the_reference_model(n, rows, cols):
    """The two layers in float64 and eval mode on table-valued input against the reference with unrounded operands and
    the rounding of mid switched off."""
    layer0, layer1 = sr.stem_layers(seed=20)
    layer0, layer1 = layer0.double().eval(), layer1.double().eval()
    image = np.random.default_rng(21).integers(0, 256, (n, rows, cols, 3)).astype(np.uint8)
    lut = sr.input_table("bfloat16")
    x = sr.lookup(image, lut)
    with torch.no_grad():
        want_mid = layer0(x)
        want = layer1(want_mid.clone())
    mid = sr.mid_reference(image, lut, layer0[0].weight.detach().numpy(), *_fold64(layer0[1]), None)
    out = sr.out_reference(mid["ref"], layer1[0].weight.detach().numpy(), *_fold64(layer1[1]), None)
    assert mid["ref"].shape == (n, 16, rows, cols) == out["ref"].shape
    assert np.allclose(mid["ref"], want_mid.numpy(), rtol=1e-12, atol=1e-12)
    assert np.allclose(out["ref"], want.numpy(), rtol=1e-12, atol=1e-12)


def test_the_shapes_hold_the_issues_list_and_the_tile():
    for shape in [(1, 1, 1), (2, 3, 3), (1, 7, 5), (1, 16, 64), (1, 17, 65), (3, 33, 130),
                  (1, sr.TILE_ROWS, sr.TILE_COLS), (1, sr.TILE_ROWS + 1, sr.TILE_COLS + 1)]:
        assert sr.SHAPES.count(shape) == 1, shape
    assert sr.SHAPES[sr.WRONG_FORMS_SHAPE] == (1, 7, 5)


@pytest.mark.parametrize("s", range(len(sr.SHAPES)), ids=sr.SHAPE_IDS)
def test_exact_inputs_are_exact(s):
    """Both representability claims of the exact family, on the drawn data."""
    c, r = sr.exact_inputs(s), sr.exact_reference(s)
    assert set(np.unique(c["lut"]).tolist()) <= {0.0, 1.0}
    assert set(np.unique(c["m0"]).tolist()) <= {-1.0, 0.0, 1.0} and np.abs(c["m1"]).max() <= 255
    assert set(np.abs(c["scale0"]).tolist()) == {1.0} and set(np.abs(c["scale1"]).tolist()) <= {0.5, 1.0, 2.0}
    for name in ("shift0", "shift1"):
        assert np.array_equal(c[name], np.round(c[name])) and np.abs(c[name]).max() <= 4
    for dtype in sorted(sr.DTYPES):
        assert torch.equal(cr.round_half(c["w0"], dtype), torch.from_numpy(c["m0"].copy()))
        assert torch.equal(cr.round_half(c["w1"], dtype), torch.from_numpy(c["m1"] / 256.0))
        assert torch.equal(cr.round_half(c["lut"], dtype), torch.from_numpy(c["lut"].astype(np.float64)))
        # claim 1: every mid value is an integer below 256 in magnitude, a value of the half dtype
        assert np.array_equal(r["mid"], np.round(r["mid"])) and np.abs(r["mid"]).max() <= 151
        assert torch.equal(cr.round_half(r["mid"].astype(np.float32), dtype), torch.from_numpy(r["mid"].copy()))
        # the same reference from the generic path on the rounded operands
        g = sr.mid_reference(c["image"], c["lut"], c["w0"], c["scale0"], c["shift0"], dtype)
        assert np.array_equal(g["ref"], r["mid"])
        o = sr.out_reference(r["mid"], c["w1"], c["scale1"], c["shift1"], dtype)
        assert np.array_equal(o["ref"], r["out"])
    assert not np.array_equal(c["w0"].astype(np.float64), c["m0"]) or not c["m0"].any()     # (the pack call has to round)
    # claim 2: sum |w1 mid| < 2^15, every partial sum a multiple of 2^-8; the epilogue's value an fp32 value below 2^16 + 4
    assert r["a1_abs"].max() < 2.0 ** 15
    a1 = F.conv2d(torch.from_numpy(r["mid"].copy()), torch.from_numpy(c["m1"] / 256.0), padding=1).numpy()
    assert np.array_equal(a1 * 256.0, np.round(a1 * 256.0))
    pre = c["scale1"].astype(np.float64).reshape(1, -1, 1, 1) * a1 + c["shift1"].astype(np.float64).reshape(1, -1, 1, 1)
    assert np.array_equal(pre.astype(np.float32).astype(np.float64), pre) and np.abs(pre).max() < 65504
    assert np.array_equal(np.maximum(pre, 0.0), r["out"])
    if s >= 2:
        assert (r["mid"] > 0).any() and (r["mid"] == 0).any() and (r["out"] > 0).any() and (r["out"] == 0).any()


def _as_half(v, dtype):
    return torch.from_numpy(np.asarray(v, np.float32)).to(sr.DTYPES[dtype]).to(torch.float64).numpy()


def _stem_fp32(c, dtype, wrong=None):
    """The contract evaluated in fp32 on the CPU, (mid, out) as half values in float64, or one of three wrong forms."""
    lut = sr.input_table(dtype)
    x = sr.lookup(c["image"], lut).float()
    w0, w1 = cr.round_half(c["w0"], dtype).float(), cr.round_half(c["w1"], dtype).float()
    if wrong == "swapped_taps":
        w0 = w0.transpose(2, 3).contiguous()
    if wrong == "byte_padding":                    # the padding applied to the byte: lut[c][0] around the image
        xp = torch.from_numpy(lut[:, 0].copy()).view(1, 3, 1, 1).expand(x.shape[0], 3, x.shape[2] + 6, x.shape[3] + 6).clone()
        xp[:, :, 3:-3, 3:-3] = x
        a0 = F.conv2d(xp, w0)
    else:
        a0 = F.conv2d(x, w0, padding=3)
    s0, h0 = (torch.from_numpy(c[k].copy()).view(1, -1, 1, 1) for k in ("scale0", "shift0"))
    mid = torch.from_numpy(_as_half(torch.clamp_min(s0 * a0 + h0, 0).numpy(), dtype)).float()
    if wrong == "computed_halo":                   # mid outside the image as relu(shift0) instead of 0
        mp = torch.clamp_min(h0, 0).expand(mid.shape[0], 16, mid.shape[2] + 2, mid.shape[3] + 2).clone()
        mp = torch.from_numpy(_as_half(mp.numpy(), dtype)).float()
        mp[:, :, 1:-1, 1:-1] = mid
        a1 = F.conv2d(mp, w1)
    else:
        a1 = F.conv2d(mid, w1, padding=1)
    s1, h1 = (torch.from_numpy(c[k].copy()).view(1, -1, 1, 1) for k in ("scale1", "shift1"))
    out = _as_half(torch.clamp_min(s1 * a1 + h1, 0).numpy(), dtype)
    return mid.double().numpy(), out


def _ratios(c, dtype, mid, out):
    """(err / tol_half of mid against the reference from the bytes, of out against the reference on this mid)."""
    rm = sr.mid_reference(c["image"], sr.input_table(dtype), c["w0"], c["scale0"], c["shift0"], dtype)
    ro = sr.out_reference(mid, c["w1"], c["scale1"], c["shift1"], dtype)
    return float((np.abs(mid - rm["ref"]) / rm["tol_half"]).max()), float((np.abs(out - ro["ref"]) / ro["tol_half"]).max())


@pytest.mark.parametrize("dtype", sorted(sr.DTYPES))
def test_bound_catches_three_wrong_forms_and_passes_fp32(dtype):
    """At (1, 7, 5): an fp32 evaluation of the contract stays inside the bound; a mid halo computed as relu(shift0),
    padding applied to the byte, and w0 with ky and kx swapped are each more than ten times outside it -- the first in
    `out` (against the reference on its own, correct, mid), the other two in `mid`."""
    s = sr.WRONG_FORMS_SHAPE
    c = sr.random_inputs(s)
    assert (c["shift0"] > 0.25).sum() * 4 >= c["shift0"].size                 # the family's condition, on the drawn data
    good_mid, good_out = _ratios(c, dtype, *_stem_fp32(c, dtype))
    assert good_mid <= 1.0 and good_out <= 1.0, (good_mid, good_out)
    mid, out = _stem_fp32(c, dtype, wrong="computed_halo")
    bad = _ratios(c, dtype, mid, out)
    assert bad[0] <= 1.0 and bad[1] > 10, bad
    for wrong in ("byte_padding", "swapped_taps"):
        bad = _ratios(c, dtype, *_stem_fp32(c, dtype, wrong=wrong))
        assert bad[0] > 10, (wrong, bad)


@pytest.mark.parametrize("s", range(len(sr.SHAPES)), ids=sr.SHAPE_IDS)
def test_fp32_evaluation_stays_inside_the_bound_at_every_shape(s):
    c = sr.random_inputs(s)
    assert (c["shift0"] > 0.25).sum() * 4 >= c["shift0"].size
    for dtype in sorted(sr.DTYPES):
        ratios = _ratios(c, dtype, *_stem_fp32(c, dtype))
        assert max(ratios) <= 1.0, ratios
        r = sr.random_mid_reference(s, dtype)
        assert (r["ref"] > 0).any() and ((r["ref"] == 0).any() or s == 0)     # ReLU cuts some and not all


def test_ulp_half_is_the_formats_spacing():
    for dtype, td in sr.DTYPES.items():
        for v in (1.0, 1.5, 1.999, 2.0, 0.75, 100.0, 3e-5, 1e-7, 0.0, 40000.0):
            t = torch.tensor(v, dtype=torch.float32).to(td)
            above = (t.view(torch.int16) + 1).view(td)                         # the next value of the format
            assert sr.ulp_half(float(t), dtype) == float(above.double() - t.double()), (dtype, v)


# ---- cnn.DrnStem: every refusal is made before anything is packed, so none needs a device ----

def _layers(**kw):
    return sr.stem_layers(seed=30, **kw)


def _changed_conv(which, **kw):
    layer0, layer1 = _layers()
    layer = (layer0, layer1)[which]
    old = layer[0]
    args = dict(in_channels=old.in_channels, out_channels=16, kernel_size=old.kernel_size, stride=1, padding=old.padding,
                bias=False)
    args.update(kw)
    layer[0] = torch.nn.Conv2d(**args)
    return layer0.eval(), layer1.eval()


def _training_bn(which):
    layer0, layer1 = _layers()
    (layer0, layer1)[which][1].train()
    return layer0, layer1


def _basic_block_layer1():
    layer0, _ = _layers()
    return layer0, torch.nn.Sequential(cb.Block(16, 16, dilation=(1, 1), seed=31)).eval()


REFUSALS = [
    (lambda: _changed_conv(0, kernel_size=3, padding=1), r"layer0's conv must be Conv2d\(3, 16, kernel_size=7"),
    (lambda: _changed_conv(0, stride=2), "layer0's conv must be"),
    (lambda: _changed_conv(0, padding=2), "layer0's conv must be"),
    (lambda: _changed_conv(1, kernel_size=1, padding=0), r"layer1's conv must be Conv2d\(16, 16, kernel_size=3"),
    (lambda: _changed_conv(1, stride=2), "layer1's conv must be"),
    (lambda: _changed_conv(1, padding=2, dilation=2), "layer1's conv must be"),
    (lambda: _changed_conv(0, bias=True), "layer0's conv has a bias"),
    (lambda: _changed_conv(1, bias=True), "layer1's conv has a bias"),
    (lambda: _layers(layer1_convs=2), r"layer1 has 6 modules.*layers\[0\] > 1"),
    (lambda: _basic_block_layer1(), "layer1 holds a BasicBlock"),
    (lambda: _training_bn(0), "eval"),
    (lambda: _training_bn(1), "eval"),
]


@pytest.mark.parametrize("make, message", REFUSALS)
def test_drn_stem_refusals_need_no_device(make, message, monkeypatch):
    def touched(*args, **kwargs):
        raise AssertionError("weights were packed before the refusal")
    monkeypatch.setattr(core, "stem_pack_weights", touched)
    with pytest.raises(core.CoreError, match=message):
        cnn.DrnStem(*make(), sr.MEAN, sr.STD)


def test_an_accepted_stem_reaches_the_packer(monkeypatch):
    """(the refusals above are not an artefact of the layers' builder)"""
    def touched(*args, **kwargs):
        raise AssertionError("reached the packer")
    monkeypatch.setattr(core, "stem_pack_weights", touched)
    with pytest.raises(AssertionError, match="reached the packer"):
        cnn.DrnStem(*_layers(), sr.MEAN, sr.STD)
    with pytest.raises(core.CoreError, match="nine"):
        cnn.Drn.from_base(torch.nn.Sequential(*_layers()), None, 19, 32, sr.MEAN, sr.STD)


SIGNATURES = [
    (core.stem_packed_bytes, "(dtype)"),
    (core.stem_pack_weights, "(w0, w1, dtype, device=0)"),
    (core.stem_ptr, "(stream=0, **fields)"),
    (core.stem, "(image, lut, packed, scale0, shift0, scale1, shift1, want_mid=False, canary=0)"),
    (cnn.input_table, "(mean, std, dtype)"),
    (cnn.DrnStem.__init__, "(self, layer0, layer1, mean, std, dtype=torch.bfloat16, device=0)"),
    (cnn.DrnStem.forward, "(self, image, want_mid=False)"),
    (cnn.Drn.__init__, "(self, layer0, layer1, layer2, layer3, layer4, layer5, layer6, layer7, layer8, seg, n_classes, "
                       "rows_power2_segmentation, mean, std, clamp=None, dtype=torch.bfloat16, device=0)"),
    (cnn.Drn.from_base, "(base, seg, n_classes, rows_power2_segmentation, mean, std, clamp=None, dtype=torch.bfloat16, "
                        "device=0)"),
    (cnn.Drn.forward, "(self, image, want_cnn_out=False)"),
]


@pytest.mark.parametrize("fn, signature", SIGNATURES, ids=[fn.__qualname__ for fn, _ in SIGNATURES])
def test_public_signatures_are_pinned(fn, signature):
    assert str(inspect.signature(fn)) == signature
