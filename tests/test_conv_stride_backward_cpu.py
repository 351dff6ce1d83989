"""The backward pass of conv + BatchNorm (+ residual) (+ ReLU) at stride 2 (f22) without a GPU: the symbols and bindings,
the struct layout against a compiled offsetof probe, every refusal of is_conv_bn_stride_backward (all made before the
device is touched), stride 1 forwarding to is_conv_bn_backward's checker message for message, the scratch size, the
reference of tests/conv_stride_backward_reference.py pinned against float64 torch.autograd, the exact family really
being exact, and the CoreErrors of the training modules."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import conv_backward_reference as cbr
import conv_bn_reference as cb
import conv_stride_backward_reference as csr
from instance_stixels_amd import core, training

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("is_conv_bn_stride_backward_scratch_bytes", "is_conv_bn_stride_backward")


def _last():
    return core.lib().is_last_error().decode()


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "instance_stixels_core.h")).read()
    for name in NAMES:
        assert name + "(" in header, name
        assert name in core.EXPORTS and hasattr(core.lib(), name), name
    for name in ("conv_bn_stride_backward", "conv_bn_stride_backward_ptr", "conv_bn_stride_backward_scratch_bytes"):
        assert callable(getattr(core, name)), name
    band = int(re.search(r"#define IS_CONV_BACKWARD_STRIDE_BAND (\d+)", header).group(1))
    assert band == core.CONV_BACKWARD_STRIDE_BAND == csr.BAND and band in (8, 16, 32)
    assert header.index("---- f21:") < header.index("---- f22:") < header.index("---- f9:")
    for cls in (training.StridedConvBnReLU, training.StridedBasicBlock, training.DrnLayers):
        assert issubclass(cls, torch.nn.Module)


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "instance_stixels_core.h"
#define F(f) printf(#f " %zu %zu\n", offsetof(is_conv_bn_stride_backward_args, f), sizeof(((is_conv_bn_stride_backward_args*)0)->f));
int main() {
    printf(". %zu 0\n", sizeof(is_conv_bn_stride_backward_args));
    FIELDS
    return 0;
}
"""


def test_args_layout_matches_the_header(tmp_path):
    cls = core.ConvBnStrideBackwardArgs
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
    # f21's struct with rows_in / cols_in for rows8 / cols8 and `stride` added behind `kernel`
    old = [n for n, _ in core.ConvBnBackwardArgs._fields_]
    new = [n for n, _ in cls._fields_]
    assert [{"rows_in": "rows8", "cols_in": "cols8"}.get(n, n) for n in new if n != "stride"] == old
    assert new[new.index("kernel") + 1] == "stride"


# A stride-2 call that would be accepted (the pointers are never dereferenced on the host: every case below is refused
# before the device is touched).  2 frames of 32 -> 64 channels, 13 x 17 in, 7 x 9 out: 63 output cells, 4032 gradient
# elements per frame; 2 * 32 * 221 * 2 = 28288 bytes of features.
BIG = 1 << 40
F16, BF16, F32 = core.HEAD_F16, core.HEAD_BF16, core.HEAD_F32
GOOD = dict(d_features=0x100000, dtype=F16, n_images=2, channels_in=32, channels_out=64, rows_in=13, cols_in=17, kernel=3,
            stride=2, dilation=1, d_weight=0x200000, d_scale=0x300000, d_out=0x400000, out_dtype=F16, relu=1,
            d_grad_out=0x500000, grad_out_dtype=F32, grad_image_stride=4032, d_grad_features=0x600000,
            grad_features_dtype=F16, d_grad_features_add=0x700000, d_grad_weight=0x800000, d_grad_scale=0x900000,
            d_grad_shift=0xa00000, d_grad_pre=0xb00000, d_scratch=0x10000000, scratch_bytes=BIG)
NEED = core.conv_bn_stride_backward_scratch_bytes(2, 32, 64, 13, 17, 3, 2, F16) if os.path.exists(core.LIB_PATH) else 0

REFUSALS = [
    # everything f21 refuses
    (dict(d_features=None), "null"),
    (dict(d_weight=None), "null"),
    (dict(d_scale=None), "null"),
    (dict(d_grad_out=None), "null"),
    (dict(d_out=None), "null d_out"),
    (dict(dtype=F32), "dtype"),
    (dict(dtype=7), "dtype"),
    (dict(channels_in=24), "channels_in"),
    (dict(channels_in=0), "channels_in"),
    (dict(channels_in=4096), "channels_in"),
    (dict(channels_out=48), "channels_out"),
    (dict(channels_out=4096), "channels_out"),
    (dict(kernel=2), "kernel"),
    (dict(kernel=5), "kernel"),
    (dict(n_images=0), "n_images"),
    (dict(n_images=65536), "n_images"),
    (dict(rows_in=0), "rows_in and cols_in"),
    (dict(cols_in=32768), "rows_in and cols_in"),
    (dict(stride=1, dilation=0), "dilation outside"),
    (dict(stride=1, dilation=9), "dilation outside"),
    (dict(stride=1, kernel=1, dilation=2), "dilation must be 1 with kernel 1"),
    (dict(relu=2), "relu"),
    (dict(out_dtype=BF16), "out_dtype"),
    (dict(d_grad_features=None, d_grad_features_add=None, d_grad_weight=None, d_grad_scale=None, d_grad_shift=None,
          d_grad_pre=None), "all null"),
    (dict(d_grad_features=None), "d_grad_features_add without"),
    (dict(grad_out_dtype=BF16), "grad_out_dtype"),
    (dict(grad_features_dtype=BF16), "grad_features_dtype"),
    (dict(grad_image_stride=4031), "grad_image_stride"),         # the OUTPUT's planes: 64 * 7 * 9
    # the stride
    (dict(stride=0), "stride is neither 1 nor 2"),
    (dict(stride=3), "stride is neither 1 nor 2"),
    (dict(dilation=2), "dilation must be 1 with stride 2"),
    # dX with channels_in % 32: layer2's 16 channels
    (dict(channels_in=16), "channels_in % 32"),
    (dict(channels_in=48), "channels_in % 32"),
    # misalignment
    (dict(d_features=0x100001), "aligned"),
    (dict(d_out=0x400001), "aligned"),
    (dict(out_dtype=F32, d_out=0x400002), "aligned"),
    (dict(d_grad_out=0x500002), "aligned"),
    (dict(d_grad_features=0x600001), "aligned"),
    (dict(grad_features_dtype=F32, d_grad_features=0x600002), "aligned"),
    (dict(d_grad_features_add=0x700001), "aligned"),
    (dict(d_grad_pre=0xb00001), "aligned"),
    (dict(d_weight=0x200002), "aligned"),
    (dict(d_grad_shift=0xa00002), "aligned"),
    # overlaps: the input-shaped operands at the INPUT's size, the output-shaped ones at the OUTPUT's
    (dict(d_grad_features=0x100000 + 28286), "overlap an input"),
    (dict(d_grad_features=0x100000 - 28286), "overlap an input"),
    (dict(d_grad_pre=0x400000 + 2 * 4032 * 2 - 2), "overlap an input"),
    (dict(d_grad_pre=0x500000 + 2 * 4032 * 4 - 2), "overlap an input"),
    (dict(d_grad_weight=0x200000 + 64 * 32 * 9 * 4 - 4), "overlap an input"),
    (dict(d_grad_features=0x700000 + 28286), "overlap an input"),
    (dict(d_grad_pre=0x600000 + 28286), "two outputs"),
    (dict(d_grad_scale=0xa00000 - 252), "two outputs"),
    (dict(d_scratch=0x100000), "overlap"),
    # scratch
    (dict(d_scratch=None), "null d_scratch"),
    (dict(d_scratch=0x10000008), "16-byte"),
    (dict(scratch_bytes=NEED - 1), "scratch_bytes"),
    # last
    (dict(reserved=(0, 0, 1, 0)), "reserved"),
]


@pytest.mark.parametrize("change, message", REFUSALS)
def test_refusals_need_no_device(change, message):
    rc = core.conv_bn_stride_backward_ptr(**dict(GOOD, **change))
    assert rc == -1                                                          # IS_EINVAL
    assert re.search(message, _last()), _last()


def test_the_good_call_fails_for_nothing_but_what_is_changed():
    # the spans that just do not overlap are accepted up to the reserved field, which is the last refusal
    for change in (dict(d_grad_features=0x100000 + 28288), dict(d_grad_pre=0x400000 + 2 * 4032 * 2),
                   dict(d_grad_pre=0x600000 + 28288), dict(scratch_bytes=NEED), dict(channels_in=16, d_grad_features=None,
                                                                                   d_grad_features_add=None)):
        assert core.conv_bn_stride_backward_ptr(**dict(GOOD, reserved=(1, 0, 0, 0), **change)) == -1
        assert "reserved" in _last(), (change, _last())
    assert core.conv_bn_stride_backward_ptr(**dict(GOOD, reserved=(1, 0, 0, 0), d_scratch=0x10000008)) == -1
    assert "16-byte" in _last()
    assert core.lib().is_conv_bn_stride_backward(None, None) == -1
    assert "null args" in _last()


# f21's accepted call, in both structs
OLD = dict(d_features=0x100000, dtype=F16, n_images=2, channels_in=32, channels_out=64, rows8=7, cols8=9, kernel=3,
           dilation=2, d_weight=0x200000, d_scale=0x300000, d_out=0x400000, out_dtype=F16, relu=1,
           d_grad_out=0x500000, grad_out_dtype=F32, grad_image_stride=4032, d_grad_features=0x600000,
           grad_features_dtype=F16, d_grad_features_add=0x700000, d_grad_weight=0x800000, d_grad_scale=0x900000,
           d_grad_shift=0xa00000, d_grad_pre=0xb00000, d_scratch=0x10000000, scratch_bytes=BIG)


def _as_stride1(fields):
    new = {{"rows8": "rows_in", "cols8": "cols_in"}.get(k, k): v for k, v in fields.items()}
    return dict(new, stride=1)


def test_stride_1_is_is_conv_bn_backward_message_for_message():
    """One checker: every refusal of f21's own CPU test gives the same message through either entry point, with the
    extents in the entry point's own names."""
    import test_conv_backward_cpu as old
    changes = [mark.args[1] for mark in old.test_refusals_need_no_device.pytestmark if mark.name == "parametrize"][0]
    assert len(changes) > 50
    for change, _ in changes + [(dict(reserved=(1, 0, 0, 0), d_scratch=0x10000008), "")]:
        assert core.conv_bn_backward_ptr(**dict(OLD, **change)) == -1
        first = _last()
        assert core.conv_bn_stride_backward_ptr(**_as_stride1(dict(OLD, **change))) == -1
        assert _last() == first.replace("rows8 and cols8", "rows_in and cols_in"), (change, first, _last())


def test_scratch_bytes():
    sb = core.conv_bn_stride_backward_scratch_bytes
    for bad in ((0, 32, 64, 7, 9, 3, 2, F16), (65536, 32, 64, 7, 9, 3, 2, F16), (1, 24, 64, 7, 9, 3, 2, F16),
                (1, 32, 48, 7, 9, 3, 2, F16), (1, 32, 64, 0, 9, 3, 2, F16), (1, 32, 64, 7, 32768, 3, 2, F16),
                (1, 32, 64, 7, 9, 2, 2, F16), (1, 32, 64, 7, 9, 3, 2, F32), (1, 32, 64, 7, 9, 3, 0, F16),
                (1, 32, 64, 7, 9, 3, 3, F16), (65535, 2048, 2048, 32767, 9, 3, 2, F16)):
        assert sb(*bad) == 0, bad
    al = lambda b: (b + 15) // 16 * 16
    B = core.CONV_BACKWARD_STRIDE_BAND

    def want(n, cin, cout, Hi, Wi, k):
        taps, Ho, Wo = k * k, (Hi + 1) // 2, (Wi + 1) // 2
        P = Ho * Wo
        return (al(n * cout * P * 2) + al(cin * cout * taps * 2) + 2 * al(cin * 4) + al(n * cout * ((P + 2047) // 2048) * 8)
                + al(cout * cin * taps * 8) + al(n * ((Ho + B - 1) // B) * taps * cout * cin * 4))

    for shape in ((2, 32, 64, 13, 17, 3), (3, 48, 32, 4 * B + 9, 33, 1), (1, 16, 32, 1024, 2048, 3), (4, 64, 128, 256, 512, 1)):
        assert sb(*shape, 2, F16) == sb(*shape, 2, BF16) == want(*shape), shape
    for shape in ((2, 32, 64, 7, 9, 3), (3, 48, 32, 69, 33, 1), (1, 512, 512, 16, 32, 3)):
        assert sb(*shape, 1, F16) == core.conv_bn_backward_scratch_bytes(*shape, F16) > 0, shape


@pytest.mark.parametrize("kernel", csr.KERNELS)
@pytest.mark.parametrize("s", [0, 1, 2, 3, 4, 6], ids=lambda s: csr.SHAPE_IDS[s])
@pytest.mark.parametrize("relu, with_res", [(True, True), (True, False), (False, True)])
def test_reference_equals_float64_autograd_on_exact_inputs(s, kernel, relu, with_res):
    """On the exact family the half rounding changes no operand, scale is a power of two and every sum is exact: the
    reference must BE float64 autograd of relu(scale conv2d(x, w, stride = 2) + shift + res)."""
    c = csr.exact_inputs(s, kernel)
    w = c["m"] / 256.0
    res = c["res"] if with_res else None
    ag = csr.autograd64(c["x"], w, c["scale"], c["shift"], res, c["dy"], kernel, relu=relu)
    assert ag["out"].shape[2:] == csr.out_extents(s)
    for dtype in csr.DTYPES:
        out_half = torch.from_numpy(ag["out"]).to(csr.DTYPES[dtype])
        assert torch.equal(out_half.double() > 0, torch.from_numpy(ag["out"]) > 0)
        gh = cbr.masked_gradient(c["dy"], out_half, relu, dtype)
        if with_res:
            assert np.array_equal(gh.double().numpy(), ag["dres"])              # gh IS the residual's gradient
        r = csr.backward(c["x"], c["w"], c["scale"], gh, kernel, dtype)
        for name in ("dx", "dw", "dscale", "dshift"):
            assert np.array_equal(r[name], ag[name]), (name, dtype)
        if kernel == 1:                                                         # nothing reaches the other three classes
            assert not r["dx"][:, :, 1::2].any() and not r["dx"][:, :, :, 1::2].any()


def test_the_reference_is_the_contracts_sum_written_out():
    """dX and G by the header's index formulas, as plain loops, on one small odd shape."""
    rng = np.random.default_rng(3)
    n, cin, cout, Hi, Wi = 1, 2, 3, 5, 7
    Ho, Wo = 3, 4
    x, w = rng.integers(0, 4, (n, cin, Hi, Wi)).astype(np.float32), rng.integers(-3, 4, (cout, cin, 3, 3)).astype(np.float32)
    gh, scale = rng.integers(-2, 3, (n, cout, Ho, Wo)).astype(np.float32), np.array([1.0, -2.0, 0.5], np.float32)
    r = csr.backward(x, w, scale, gh, 3, "float16")
    dx, Gs = np.zeros((n, cin, Hi, Wi)), np.zeros((cout, cin, 3, 3))
    for co in range(cout):
        for ci in range(cin):
            for ky in range(3):
                for kx in range(3):
                    for y in range(Ho):
                        for xo in range(Wo):
                            rr, cc = 2 * y + ky - 1, 2 * xo + kx - 1
                            if 0 <= rr < Hi and 0 <= cc < Wi:
                                Gs[co, ci, ky, kx] += gh[0, co, y, xo] * x[0, ci, rr, cc]
                                dx[0, ci, rr, cc] += scale[co] * w[co, ci, ky, kx] * gh[0, co, y, xo]
    assert np.array_equal(r["G"], Gs) and np.array_equal(r["dx"], dx)
    assert csr.taps_of_class(3, 3, 3).tolist() == [[1, 2, 1], [2, 4, 2], [1, 2, 1]]


@pytest.mark.parametrize("kernel", csr.KERNELS)
@pytest.mark.parametrize("s", range(len(csr.SHAPES)), ids=csr.SHAPE_IDS)
def test_the_exact_family_is_exact_in_both_dtypes(s, kernel):
    c = csr.exact_inputs(s, kernel)
    n, cin, cout, Hi, Wi = csr.SHAPES[s]
    Ho, Wo = csr.out_extents(s)
    assert c["dy"].shape == c["res"].shape == (n, cout, Ho, Wo) and c["add"].shape == c["x"].shape == (n, cin, Hi, Wi)
    for dtype in csr.DTYPES:
        td = csr.DTYPES[dtype]
        for name in ("x", "dy", "add", "res"):
            assert torch.equal(torch.from_numpy(c[name].copy()).to(td).float(), torch.from_numpy(c[name].copy())), name
        assert np.array_equal(torch.from_numpy(c["w"].copy()).to(td).double().numpy(), c["m"] / 256.0)
        ws = cbr.scaled_weight(c["w"], c["scale"], dtype).numpy()
        assert np.array_equal(ws, c["scale"].astype(np.float64).reshape(-1, 1, 1, 1) * c["m"] / 256.0)
    # every partial sum of a chunk stays below 2^24: at most min(BAND, rows_out) * cols_out products of at most 3 * 2
    assert min(csr.BAND, Ho) * Wo * 6 < 2 ** 24
    # the forward's sums (they decide the ReLU mask): f18's claim, at most taps * channels_in products of at most 3
    assert kernel * kernel * cin * 3 * 2 * 2 ** 9 < 2 ** 24
    # dX: at most 4 * channels_out products of at most 2 * 2, multiples of 2^-9, plus the add of at most 8
    assert (4 * cout * 4 + 8) * 2 ** 9 < 2 ** 24
    # dscale: multiples of 2^-8 below 2^53 in binary64
    assert cin * kernel * kernel * n * Ho * Wo * 6 * 2 ** 8 < 2 ** 53


def _pair(stride=2, dilation=1, train=False, cin=32):
    conv = torch.nn.Conv2d(cin, 32, 3, stride=stride, padding=dilation, dilation=dilation, bias=False)
    bn = torch.nn.BatchNorm2d(32)
    return conv, (bn.train() if train else bn.eval())


def _layers(width=32, cin=16):
    seq = lambda ci, co, s, d: torch.nn.Sequential(torch.nn.Conv2d(ci, co, 3, stride=s, padding=d, dilation=d, bias=False),
                                                   cb.batchnorm(co, 40 + d), torch.nn.ReLU())
    blocks = lambda stride, d, down, seed: torch.nn.Sequential(
        cb.Block(width, width, dilation=d, downsample=down, stride=stride, seed=seed),
        cb.Block(width, width, dilation=d, seed=seed + 5))
    return [seq(cin, width, 2, 1), blocks(2, (1, 1), True, 50), blocks(2, (1, 1), True, 60), blocks(1, (2, 2), True, 70),
            blocks(1, (4, 4), False, 80), seq(width, width, 1, 2), seq(width, width, 1, 1)]


def test_the_modules_refuse_what_they_do_not_cover():
    layer = training.StridedConvBnReLU(*_pair())
    assert layer.stride == 2 and {n for n, _ in layer.named_parameters()} == {"weight", "bn.weight", "bn.bias"}
    assert training.StridedConvBnReLU(*_pair(stride=1, dilation=2)).stride == 1
    with pytest.raises(core.CoreError, match="stride 2 needs dilation 1"):
        training.StridedConvBnReLU(*_pair(dilation=2))
    with pytest.raises(core.CoreError, match="stride"):
        training.StridedConvBnReLU(*_pair(stride=3))
    with pytest.raises(core.CoreError, match="batch statistics"):
        training.StridedConvBnReLU(*_pair(train=True))
    with pytest.raises(core.CoreError, match="fp32 features"):
        layer(torch.zeros(1, 32, 4, 4))
    block = training.StridedBasicBlock(cb.Block(32, 64, dilation=(1, 1), downsample=True, stride=2).eval())
    assert block.stride == 2 and len(list(block.parameters())) == 9
    with pytest.raises(core.CoreError, match="fp32 features"):
        block(torch.zeros(1, 32, 4, 4))
    with pytest.raises(core.CoreError, match="Bottleneck"):
        b = cb.Block(32, 32, dilation=(1, 1), downsample=True, stride=2).eval()
        b.conv3 = b.conv2
        training.StridedBasicBlock(b)
    with pytest.raises(core.CoreError, match="batch statistics"):
        training.StridedBasicBlock(cb.Block(32, 64, dilation=(1, 1), downsample=True, stride=2).train())
    with pytest.raises(core.CoreError, match="stride 2 needs dilation 1"):
        training.StridedBasicBlock(cb.Block(32, 64, dilation=(2, 2), downsample=True, stride=2).eval())
    with pytest.raises(core.CoreError, match="no downsample"):
        training.StridedBasicBlock(cb.Block(32, 32, dilation=(1, 1), stride=2).eval())
    with pytest.raises(core.CoreError, match="residual must have the shape"):
        b = cb.Block(32, 64, dilation=(1, 1), downsample=True, stride=2).eval()
        b.downsample[0].stride = (1, 1)
        training.StridedBasicBlock(b)
    # f21's classes keep refusing stride 2
    with pytest.raises(core.CoreError, match="only the stride-1 layers"):
        training.ConvBnReLU(*_pair())
    with pytest.raises(core.CoreError, match="only the stride-1 layers"):
        training.BasicBlock(cb.Block(32, 64, dilation=(1, 1), downsample=True, stride=2).eval())
    with pytest.raises(core.CoreError, match="device tensor"):
        core.conv_bn_stride_backward(torch.zeros(1, 32, 4, 4), None, None, None, None, 3, 2)


def test_drn_layers_chain_and_refuse_an_input_that_requires_grad():
    net = training.DrnLayers(*[l.eval() for l in _layers()])
    kinds = [type(m).__name__ for m in net.layers]
    assert kinds == ["StridedConvBnReLU"] + ["StridedBasicBlock"] * 8 + ["StridedConvBnReLU"] * 2
    assert [m.stride for m in net.layers] == [2, 2, 1, 2, 1, 1, 1, 1, 1, 1, 1]
    assert len(list(net.parameters())) == 3 + 3 * 9 + 5 * 6 + 2 * 3
    with pytest.raises(core.CoreError, match="fp32 features"):
        net(torch.zeros(1, 16, 8, 8))
    with pytest.raises(core.CoreError, match="requires grad: the stem is frozen"):        # before any launch
        net(torch.zeros(1, 16, 8, 8, dtype=torch.float16, requires_grad=True))
    with pytest.raises(core.CoreError, match="batch statistics"):
        training.DrnLayers(*[l.train() for l in _layers()])
    with pytest.raises(core.CoreError, match="nn.Sequential"):
        training.DrnLayers(torch.nn.ReLU(), *_layers()[1:])
