"""The backward pass of the stem (f23) without a GPU: the symbols and bindings, the struct layout against a compiled
offsetof probe, the constants against the header, every refusal of is_stem_backward (all made before the device is
touched), the scratch size, the Python refusals, the reference of tests/stem_backward_reference.py pinned against
float64 torch.autograd, an fp32 evaluation of the contract inside the bounds, three wrong forms outside them, the exact
family really being exact, and the masks being exercised."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.grad as G

import stem_backward_reference as sbr
import stem_reference as sr
from instance_stixels_amd import core, training

ROOT = sbr.ROOT
HEADER = sbr.HEADER
KERNEL_FILE = os.path.join(ROOT, "instance_stixels_amd", "csrc", "is_k_stem_backward.hip")
DTYPE_NAMES = sorted(sbr.DTYPES)


def test_symbols_are_declared_exported_and_bound():
    header = open(HEADER).read()
    for name in ("is_stem_backward_scratch_bytes", "is_stem_backward", "is_stem_backward_constant"):
        assert name + "(" in header and name in core.EXPORTS and hasattr(core.lib(), name), name
    for fn in ("stem_backward_scratch_bytes", "stem_backward_ptr", "stem_backward"):
        assert callable(getattr(core, fn)), fn
    assert issubclass(core.StemBackwardArgs, ctypes.Structure)
    assert issubclass(training.Stem, torch.nn.Module)
    assert header.index("---- f22:") < header.index("---- f23:")
    assert "is_k_stem_backward.hip" in open(os.path.join(ROOT, "instance_stixels_amd", "csrc", "Makefile")).read()
    want = ("image", "lut", "w0", "w1", "scale0", "scale1", "mid", "out", "grad_out", "grad_next", "weight_next",
            "scale_next", "want_weight0", "want_scale0", "want_shift0", "want_weight1", "want_scale1", "want_shift1",
            "want_pre", "canary")
    assert tuple(inspect.signature(core.stem_backward).parameters) == want


def test_constants_come_from_the_library_and_match_the_header():
    assert core.STEM_BACKWARD_BAND == sbr.BAND and core.STEM_BACKWARD_SEGMENT == sbr.SEGMENT
    assert core.STEM_BACKWARD_TILE_ROWS == sbr.TILE_ROWS and core.STEM_BACKWARD_TILE_COLS == sbr.TILE_COLS
    assert core.lib().is_stem_backward_constant(4) == -1
    kernel = open(KERNEL_FILE).read()
    for name in ("IS_STEM_BACKWARD_BAND", "IS_STEM_BACKWARD_SEGMENT", "IS_STEM_BACKWARD_TILE_ROWS",
                 "IS_STEM_BACKWARD_TILE_COLS"):
        assert name in kernel, name                        # the kernels take them from the header, not from a literal
    assert sbr.SEGMENT % 32 == 0
    # the shapes reach a second and a third band, a second segment and a second tile both ways
    assert (1, sbr.BAND + 1, 9) in sbr.SHAPES and (2, 2 * sbr.BAND + 3, 5) in sbr.SHAPES
    assert (1, 3, sbr.SEGMENT + 1) in sbr.SHAPES and (1, sbr.TILE_ROWS + 1, sbr.TILE_COLS + 1) in sbr.SHAPES
    assert all(s in sbr.SHAPES for s in sr.SHAPES)


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "instance_stixels_core.h"
#define F(f) printf(#f " %zu %zu\n", offsetof(is_stem_backward_args, f), sizeof(((is_stem_backward_args*)0)->f));
int main() {
    printf(". %zu 0\n", sizeof(is_stem_backward_args));
    FIELDS
    return 0;
}
"""


def test_args_layout_matches_the_header(tmp_path):
    cls = core.StemBackwardArgs
    (tmp_path / "probe.cpp").write_text(PROBE.replace("FIELDS", "".join(f"F({n})" for n, _ in cls._fields_)))
    exe = str(tmp_path / "probe")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "probe.cpp"), "-o", exe],
                   check=True)
    got = {f: (int(off), int(size)) for f, off, size in
           (l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())}
    assert got["."][0] == ctypes.sizeof(cls)
    for name, _ in cls._fields_:
        field = getattr(cls, name)
        assert got[name] == (field.offset, field.size), name


# A call that would be accepted (the pointers are never dereferenced on the host: every case below is refused before
# the device is touched).  2 frames of 7 x 9: 63 pixels, 1008 gradient elements per frame, 378 bytes of image.
BIG = 1 << 40
F16, BF16, F32 = core.HEAD_F16, core.HEAD_BF16, core.HEAD_F32
GOOD = dict(d_image=0x100000, n_images=2, rows=7, cols=9, d_lut=0x110000, dtype=F16, d_w0=0x200000, d_w1=0x210000,
            d_scale0=0x300000, d_scale1=0x310000, d_mid=0x400000, d_out=0x410000, d_grad_out=0x500000,
            grad_out_dtype=F32, grad_image_stride=1008, d_grad_weight0=0x800000, d_grad_scale0=0x810000,
            d_grad_shift0=0x820000, d_grad_weight1=0x830000, d_grad_scale1=0x840000, d_grad_shift1=0x850000,
            d_grad_pre1=0xb00000, d_grad_pre0=0xb10000, d_scratch=0x10000000, scratch_bytes=BIG)
NEXT = dict(d_grad_out=None, d_grad_next=0x600000, channels_next=32, d_weight_next=0x610000, d_scale_next=0x620000)
NEED = core.stem_backward_scratch_bytes(2, 7, 9, 0, F16) if os.path.exists(core.LIB_PATH) else 0
NEED_NEXT = core.stem_backward_scratch_bytes(2, 7, 9, 32, F16) if os.path.exists(core.LIB_PATH) else 0
OUTPUTS = ("d_grad_weight0", "d_grad_scale0", "d_grad_shift0", "d_grad_weight1", "d_grad_scale1", "d_grad_shift1",
           "d_grad_pre1", "d_grad_pre0")


@pytest.mark.parametrize("change, message", [
    # everything is_stem refuses for the fields they share
    (dict(d_image=None), "null"),
    (dict(d_lut=None), "null"),
    (dict(d_w0=None), "null"),
    (dict(d_w1=None), "null"),
    (dict(d_scale0=None), "null"),
    (dict(d_scale1=None), "null"),
    (dict(d_mid=None), "null"),
    (dict(d_out=None), "null"),
    (dict(dtype=F32), "dtype"),
    (dict(dtype=7), "dtype"),
    (dict(n_images=0), "n_images"),
    (dict(n_images=65536), "n_images"),
    (dict(rows=0), "rows"),
    (dict(cols=32768), "cols"),
    # the gradient's source: both, neither, the second one's fields and range
    (dict(d_grad_next=0x600000), "both gradient sources"),
    (dict(channels_next=32), "both gradient sources"),
    (dict(d_grad_out=None), "no gradient source"),
    (dict(NEXT, d_weight_next=None), "null d_grad_next, d_weight_next or d_scale_next"),
    (dict(NEXT, channels_next=0), "channels_next"),
    (dict(NEXT, channels_next=16), "channels_next"),
    (dict(NEXT, channels_next=48), "channels_next"),
    (dict(NEXT, channels_next=160), "channels_next"),
    (dict(NEXT, d_scale_next=None), "null d_grad_next, d_weight_next or d_scale_next"),
    (dict(NEXT, d_grad_next=None), "null d_grad_next, d_weight_next or d_scale_next"),
    (dict(NEXT, d_grad_next=0x600001), "aligned"),
    (dict(NEXT, d_weight_next=0x610002), "aligned"),
    (dict(NEXT, d_scale_next=0x620002), "aligned"),
    # (2 * 32 * 4 * 5 * 2 = 2560 bytes of layer2's masked gradient)
    (dict(NEXT, d_grad_pre1=0x600000 + 2558), "overlap an input"),
    (dict(NEXT, d_grad_weight1=0x610000 + 32 * 144 * 4 - 4), "overlap an input"),
    (dict(NEXT, d_grad_shift0=0x620000 + 124), "overlap an input"),
    (dict(NEXT, scratch_bytes=NEED_NEXT - 1), "scratch_bytes"),
    (dict(NEXT, reserved=(0, 0, 0, 1)), "reserved"),
    (dict(grad_out_dtype=BF16), "grad_out_dtype"),
    (dict(grad_image_stride=1007), "grad_image_stride"),
    # misalignment
    (dict(d_lut=0x110001), "aligned"),
    (dict(d_mid=0x400001), "aligned"),
    (dict(d_out=0x410001), "aligned"),
    (dict(d_grad_out=0x500002), "aligned"),
    (dict(grad_out_dtype=F16, d_grad_out=0x500001), "aligned"),
    (dict(d_w0=0x200002), "aligned"),
    (dict(d_w1=0x210002), "aligned"),
    (dict(d_scale0=0x300002), "aligned"),
    (dict(d_scale1=0x310002), "aligned"),
    (dict(d_grad_weight0=0x800002), "aligned"),
    (dict(d_grad_shift1=0x850002), "aligned"),
    (dict(d_grad_pre1=0xb00001), "aligned"),
    (dict(d_grad_pre0=0xb10001), "aligned"),
    # output bytes that overlap inputs or each other (2 * 16 * 63 * 2 = 4032 bytes of a saved tensor)
    (dict(d_grad_pre1=0x400000 + 4030), "overlap an input"),
    (dict(d_grad_pre0=0x410000), "overlap an input"),
    (dict(d_grad_pre0=0x100000 + 376), "overlap an input"),
    (dict(d_grad_pre1=0x500000 + 2 * 1008 * 4 - 2), "overlap an input"),
    (dict(d_grad_weight0=0x200000 + 16 * 147 * 4 - 4), "overlap an input"),
    (dict(d_grad_weight1=0x210000 + 16 * 144 * 4 - 4), "overlap an input"),
    (dict(d_grad_shift0=0x300000 + 60), "overlap an input"),
    (dict(d_grad_scale1=0x110000 + 1532), "overlap an input"),
    (dict(d_grad_scale0=0x820000 - 60), "two outputs"),
    (dict(d_grad_pre0=0xb00000 + 4030), "two outputs"),
    (dict(d_scratch=0x400000), "overlap"),
    (dict(d_scratch=0x830000), "overlap"),
    # scratch
    (dict(d_scratch=None), "null d_scratch"),
    (dict(d_scratch=0x10000008), "16-byte"),
    (dict(scratch_bytes=NEED - 1), "scratch_bytes"),
    # no output asked for
    ({k: None for k in OUTPUTS}, "no output"),
    # last
    (dict(reserved=(0, 0, 1, 0)), "reserved"),
])
def test_refusals_need_no_device(change, message):
    rc = core.stem_backward_ptr(**dict(GOOD, **change))
    assert rc == -1                                                          # IS_EINVAL
    assert re.search(message, core.lib().is_last_error().decode()), core.lib().is_last_error()


def test_reserved_is_the_last_refusal():
    # a call that is refused for the reserved field alone has passed every other check: the same call with another
    # fault names that fault
    assert core.stem_backward_ptr(**dict(GOOD, reserved=(1, 0, 0, 0), d_scratch=0x10000008)) == -1
    assert b"16-byte" in core.lib().is_last_error()
    assert core.stem_backward_ptr(**dict(GOOD, reserved=(1, 0, 0, 0), **{k: None for k in OUTPUTS})) == -1
    assert b"no output" in core.lib().is_last_error()
    assert core.lib().is_stem_backward(None, None) == -1 and b"null args" in core.lib().is_last_error()


def test_scratch_bytes_is_monotone_and_zero_for_refused_shapes():
    f = core.stem_backward_scratch_bytes
    assert f(0, 7, 9, 0, F16) == 0 and f(65536, 7, 9, 0, F16) == 0 and f(1, 0, 9, 0, F16) == 0
    assert f(1, 7, 32768, 0, F16) == 0 and f(1, 7, 9, 0, F32) == 0 and f(1, 7, 9, 0, 7) == 0
    assert f(1, 7, 9, 48, F16) == 0 and f(1, 7, 9, 160, F16) == 0
    assert f(1, 7, 9, 16, F16) == 0 and f(1, 7, 9, -32, F16) == 0
    # source (b) adds g_out and that layer's pack
    assert NEED_NEXT >= NEED + 2 * 16 * 63 * 2 + 9 * 16 * 32 * 2 and f(2, 7, 9, 64, F16) > NEED_NEXT
    assert f(2, 7, 9, 128, F16) > f(2, 7, 9, 96, F16) > f(2, 7, 9, 64, F16)
    assert f(2, 7, 9, 0, F16) == NEED == f(2, 7, 9, 0, BF16) and NEED % 16 == 0
    last = 0
    for n, H, W in ((1, 1, 1), (1, 7, 9), (2, 7, 9), (2, sbr.BAND + 1, 9), (2, sbr.BAND + 1, sbr.SEGMENT + 1), (3, 200, 300)):
        assert f(n, H, W, 0, F16) > last
        last = f(n, H, W, 0, F16)
    # at least gh1 and gh0 and the partials of every chunk
    n, H, W = 3, 200, 300
    assert last >= 2 * n * 16 * H * W * 2 + sbr.chunks_of(n, H, W) * (16 * 16 * 9 + 16 * 3 * 49) * 4


class _Cuda:
    """Stands in for a device tensor in the checks that come before a device is needed."""


def test_python_refusals_come_before_anything_is_packed():
    c = sbr.random_inputs(sbr.WRONG_FORMS_SHAPE)
    image = torch.from_numpy(c["image"].copy())
    with pytest.raises(core.CoreError, match="both gradient sources"):
        core.stem_backward(image, None, c["w0"], c["w1"], c["scale0"], c["scale1"], None, None, grad_out=image,
                           grad_next=image)
    with pytest.raises(core.CoreError, match="come together"):
        core.stem_backward(image, None, c["w0"], c["w1"], c["scale0"], c["scale1"], None, None, grad_next=image)
    with pytest.raises(core.CoreError, match="no gradient source"):
        core.stem_backward(image, None, c["w0"], c["w1"], c["scale0"], c["scale1"], None, None)
    with pytest.raises(core.CoreError, match="uint8 device tensor"):
        core.stem_backward(image, None, c["w0"], c["w1"], c["scale0"], c["scale1"], None, None, grad_out=image)
    layer0, layer1 = sr.stem_layers(0)
    with pytest.raises(core.CoreError, match="training mode"):
        training.Stem(layer0.train(), layer1, sr.MEAN, sr.STD, torch.float16)
    layer0.eval()
    with pytest.raises(core.CoreError, match="three"):
        training.Stem(layer0, sr.stem_layers(0, layer1_convs=2)[1], sr.MEAN, sr.STD, torch.float16)
    with pytest.raises(core.CoreError, match="dtype"):
        training.Stem(layer0, layer1, sr.MEAN, sr.STD, torch.float32)
    # training.Drn: the checks of the stem and of DrnLayers, and layer2 as the stem's backward takes it
    seq = lambda ci, co, stride: torch.nn.Sequential(torch.nn.Conv2d(ci, co, 3, stride=stride, padding=1, bias=False),
                                                     torch.nn.BatchNorm2d(co), torch.nn.ReLU()).eval()
    rest = [seq(32, 32, 1) for _ in range(6)]
    with pytest.raises(core.CoreError, match="layer2 must be"):
        training.Drn(layer0, layer1, seq(16, 32, 1), *rest, sr.MEAN, sr.STD, torch.float16)
    with pytest.raises(core.CoreError, match="multiple of 32"):
        training.Drn(layer0, layer1, seq(16, 64 + 16, 2), seq(80, 32, 1), *rest[1:], sr.MEAN, sr.STD, torch.float16)
    with pytest.raises(core.CoreError, match="nine"):
        training.Drn.from_base(torch.nn.Sequential(layer0, layer1), sr.MEAN, sr.STD)
    net = training.Drn.from_base(torch.nn.Sequential(layer0, layer1, seq(16, 32, 2), *rest), sr.MEAN, sr.STD, torch.float16)
    assert len(list(net.parameters())) == 6 + 7 * 3
    with pytest.raises(core.CoreError, match="uint8 device tensor"):
        net(image)
    assert inspect.getsource(training.DrnLayers.forward).count("the stem is frozen") == 1
    stem = training.Stem(layer0, layer1, sr.MEAN, sr.STD, torch.float16)
    assert sorted(n for n, _ in stem.named_parameters()) == ["bn0.bias", "bn0.weight", "bn1.bias", "bn1.weight",
                                                            "weight0", "weight1"]
    with pytest.raises(core.CoreError, match="uint8 device tensor"):
        stem(image)


def _outside(err, tol):
    """The largest err / tol over the elements with a bound above zero."""
    m = tol > 0
    return float((err[m] / tol[m]).max())


@pytest.mark.parametrize("s", range(len(sbr.SHAPES)), ids=sbr.SHAPE_IDS)
def test_reference_agrees_with_float64_autograd_on_unrounded_operands(s):
    """The reference's chain with no rounding anywhere (dtype None is not a half: the operands are taken as given) is
    torch's autograd of relu(bn(conv)) twice."""
    c = sbr.random_inputs(s)
    lut64 = sr.input_table("float16").astype(np.float64)
    a = sbr.autograd64(c, lut64)
    gh1 = np.where(a["out"] > 0, c["dy"].astype(np.float64), 0.0)
    wT = torch.from_numpy(c["scale1"].astype(np.float64)).view(-1, 1, 1, 1) * torch.from_numpy(c["w1"].astype(np.float64))
    dmid = G.conv2d_input(gh1.shape, wT, torch.from_numpy(gh1), padding=1).numpy()
    gh0 = np.where(a["mid"] > 0, dmid, 0.0)
    l1 = sbr.weight_gradients(torch.from_numpy(a["mid"]), c["w1"], c["scale1"], gh1, 1, None)
    l0 = sbr.weight_gradients(sr.lookup(c["image"], lut64), c["w0"], c["scale0"], gh0, 3, None)
    for layer, r in ((0, l0), (1, l1)):
        for name in ("dw", "dscale", "dshift"):
            want, got = a["%s%d" % (name, layer)], r[name]
            assert np.allclose(got, want, rtol=1e-10, atol=1e-10 * max(1.0, np.abs(want).max())), (layer, name)


def _fp32_chunked(x32, gh32, shape, padding):
    """G as the contract splits it: one float32 contraction per chunk (torch's order inside it), the partials added
    in float64."""
    n, _, H, W = gh32.shape
    total = torch.zeros(shape, dtype=torch.float64)
    for i in range(n):
        for y in range(0, H, sbr.BAND):
            for x in range(0, W, sbr.SEGMENT):
                g = torch.zeros_like(gh32)
                g[i, :, y:y + sbr.BAND, x:x + sbr.SEGMENT] = gh32[i, :, y:y + sbr.BAND, x:x + sbr.SEGMENT]
                total += G.conv2d_weight(x32, shape, g, padding=padding).double()
    return total.numpy()


def _fp32_contract(c, lut, mid, out, dtype):
    """The contract in fp32 with another summation order: torch's float32 convolutions on the half values."""
    td = sbr.DTYPES[dtype]
    gh1 = sbr.masked_gradient(c["dy"], out, dtype)
    ws = sbr.cbr.scaled_weight(c["w1"], c["scale1"], dtype).float()
    dmid = G.conv2d_input(gh1.shape, ws, gh1.float(), padding=1)
    gh0 = sbr.masked_gradient(dmid.to(td), mid, dtype)
    midt = torch.from_numpy(np.ascontiguousarray(mid, np.float32))
    x = sbr.layer0_operand(c["image"], lut, dtype).float()
    G1 = _fp32_chunked(midt, gh1.float(), (16, 16, 3, 3), 1)
    G0 = _fp32_chunked(x, gh0.float(), (16, 3, 7, 7), 3)
    return gh1, dmid.numpy(), gh0, G1, G0


@pytest.mark.parametrize("dtype", DTYPE_NAMES)
@pytest.mark.parametrize("s", range(len(sbr.SHAPES)), ids=sbr.SHAPE_IDS)
def test_an_fp32_evaluation_of_the_contract_is_inside_the_bounds(s, dtype):
    c = sbr.random_inputs(s)
    lut = sr.input_table(dtype)
    mid, out = sbr.forward_halves(c, lut, dtype)
    gh1, dmid, gh0, G1, G0 = _fp32_contract(c, lut, mid, out, dtype)
    d = sbr.data_gradient(gh1, c["w1"], c["scale1"], dtype)
    assert (np.abs(dmid - d["ref"]) <= d["tol"]).all()
    l1 = sbr.layer1_gradients(mid, c["w1"], c["scale1"], gh1, dtype)
    l0 = sbr.layer0_gradients(c["image"], lut, c["w0"], c["scale0"], gh0, dtype)
    assert (np.abs(G1 - l1["G"]) <= l1["tol_G"]).all()
    assert (np.abs(G0 - l0["G"]) <= l0["tol_G"]).all()
    # the masks are exercised
    if out.size >= 1024:
        for name, t in (("out", out), ("mid", mid)):
            share = float((t > 0).mean())
            assert 0.2 <= share <= 0.8, (name, share)


@pytest.mark.parametrize("dtype", DTYPE_NAMES)
def test_three_wrong_forms_land_ten_times_outside_their_bounds(dtype):
    s = sbr.WRONG_FORMS_SHAPE
    c = sbr.random_inputs(s)
    lut = sr.input_table(dtype)
    mid, out = sbr.forward_halves(c, lut, dtype)
    r = sbr.chain(c, lut, mid, out, dtype)
    # G0 padded with lut[c][0] instead of nothing
    padded = sbr.layer0_operand(c["image"], lut, dtype, pad_with_table=True)
    wrong = G.conv2d_weight(padded, (16, 3, 7, 7), r["gh0"].double(), padding=0).numpy()
    assert _outside(np.abs(wrong - r["l0"]["G"]), r["l0"]["tol_G"]) > 10
    # wT1 without the tap flip
    wrong = sbr.data_gradient(r["gh1"], c["w1"], c["scale1"], dtype, flip=False)["ref"]
    assert _outside(np.abs(wrong - r["dmid"]["ref"]), r["dmid"]["tol_half"]) > 10
    # a mask taken from mid >= 0: gh0 is dMid everywhere, and the gradients of layer0 follow
    everywhere = torch.from_numpy(r["dmid"]["ref"].astype(np.float32)).to(sbr.DTYPES[dtype])
    assert (mid == 0).any() and not torch.equal(everywhere, r["gh0"])
    wrong = sbr.layer0_gradients(c["image"], lut, c["w0"], c["scale0"], everywhere, dtype)
    assert _outside(np.abs(wrong["G"] - r["l0"]["G"]), r["l0"]["tol_G"]) > 10
    assert _outside(np.abs(wrong["dshift"] - r["l0"]["dshift"]), r["l0"]["tol_dshift"]) > 10


def _chunk_abs_sums(x64, gh64, shape, padding):
    """The largest absolute-value contraction of any chunk's accumulator."""
    n, _, H, W = gh64.shape
    worst = 0.0
    for i in range(n):
        for y in range(0, H, sbr.BAND):
            for x in range(0, W, sbr.SEGMENT):
                g = torch.zeros_like(gh64)
                g[i, :, y:y + sbr.BAND, x:x + sbr.SEGMENT] = gh64[i, :, y:y + sbr.BAND, x:x + sbr.SEGMENT].abs()
                worst = max(worst, float(G.conv2d_weight(x64.abs(), shape, g, padding=padding).max()))
    return worst


EXACT_CASES = [(s, 0) for s in range(len(sbr.SHAPES))] + sbr.NEXT_CASES
EXACT_IDS = sbr.SHAPE_IDS + sbr.NEXT_IDS


@pytest.mark.parametrize("s, cn", EXACT_CASES, ids=EXACT_IDS)
def test_exact_family_is_exact(s, cn):
    """Every value in front of a rounding is an integer that fp32 holds, in every order: proved per shape from the
    absolute-value contractions, not assumed.  cn > 0: source (b), with g_out from layer2's masked gradient."""
    c, r = sbr.exact_inputs(s), sbr.exact_reference(s) if cn == 0 else sbr.exact_reference_next(s, cn)
    if cn:
        nx = sbr.next_inputs(s, cn, "exact")
        for dtype in DTYPE_NAMES:
            td = sbr.DTYPES[dtype]
            assert torch.equal(torch.from_numpy(nx["w"]).to(td).double(), torch.from_numpy(nx["m"]))
            t = torch.from_numpy(r["gout"]).float()
            assert torch.equal(t.to(td).double(), torch.from_numpy(r["gout"]))
        A = G.conv2d_input(r["gout"].shape, torch.from_numpy(np.abs(nx["m"])), torch.from_numpy(np.abs(nx["gh"]).astype(np.float64)),
                           stride=2, padding=1)
        assert float(A.max()) <= 4 * cn < 65504 and (nx["gh"] == 0).mean() > 0.3
    for dtype in DTYPE_NAMES:
        td = sbr.DTYPES[dtype]
        for name in ("lut", "m0", "m1"):
            t = torch.from_numpy(np.asarray(c[name], np.float32))
            assert torch.equal(t.to(td).float(), t), name
        # the master weights round to the integers
        assert torch.equal(torch.from_numpy(c["w0"]).to(td).double(), torch.from_numpy(c["m0"]))
        assert torch.equal(torch.from_numpy(c["w1"]).to(td).double(), torch.from_numpy(c["m1"]))
        for name in ("mid", "gh1", "dmid", "gh0"):
            t = torch.from_numpy(r[name]).float()
            assert torch.equal(t.to(td).double(), torch.from_numpy(r[name])), (name, dtype)
    # the forward: integers below 2^24 in front of the rounding (stem_reference's argument, with |w1| <= 1)
    assert np.abs(r["mid"]).max() <= 151 and np.abs(r["out"]).max() < 2 ** 24
    assert (r["mid"] == np.rint(r["mid"])).all() and (r["out"] == np.rint(r["out"])).all()
    # dMid: the absolute-value contraction is below fp16's largest value (and an integer: any order is exact)
    wT = torch.from_numpy(np.abs(c["m1"]))
    A = G.conv2d_input(r["gh1"].shape, wT, torch.from_numpy(np.abs(r["gh1"])), padding=1)
    assert float(A.max()) < 65504 and float(A.max()) <= 144
    # G1 and G0: every chunk's absolute sum is below 2^24 quanta of 1
    mid64, x64 = torch.from_numpy(r["mid"].copy()), sr.lookup(c["image"], c["lut"])
    assert _chunk_abs_sums(mid64, torch.from_numpy(r["gh1"].copy()), (16, 16, 3, 3), 1) < 2 ** 24
    assert _chunk_abs_sums(x64, torch.from_numpy(r["gh0"].copy()), (16, 3, 7, 7), 3) < 2 ** 24
    # the binary64 sums are integers far below 2^53
    for name in ("dw0", "dw1", "dscale0", "dscale1", "dshift0", "dshift1"):
        assert (r[name] == np.rint(r[name])).all() and np.abs(r[name]).max() < 2 ** 50, name
    # both masks are exercised
    if r["out"].size >= 1024:
        assert 0.2 <= float((r["out"] > 0).mean()) <= 0.8 and 0.2 <= float((r["mid"] > 0).mean()) <= 0.8
