"""The backward pass of conv + BatchNorm (+ residual) (+ ReLU) (f21) without a GPU: the symbols and bindings, the
struct layout against a compiled offsetof probe, every refusal of is_conv_bn_backward (all made before the device is
touched), the scratch size, the reference of tests/conv_backward_reference.py pinned against float64 torch.autograd,
the exact family really being exact, and the CoreErrors of the training modules."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import conv_backward_reference as cbr
from instance_stixels_amd import core, training

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("is_conv_bn_backward_scratch_bytes", "is_conv_bn_backward")


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "instance_stixels_core.h")).read()
    for name in NAMES:
        assert name + "(" in header, name
        assert name in core.EXPORTS and hasattr(core.lib(), name), name
    for name in ("conv_bn_backward", "conv_bn_backward_ptr", "conv_bn_backward_scratch_bytes"):
        assert callable(getattr(core, name)), name
    band = int(re.search(r"#define IS_CONV_BACKWARD_BAND (\d+)", header).group(1))
    assert band == core.CONV_BACKWARD_BAND == cbr.BAND
    assert header.index("---- f20:") < header.index("---- f21:")
    for word in ("FROZEN", "train.py:947", "loss scaling"):
        assert word in header, word
    assert issubclass(training.ConvBnReLU, torch.nn.Module) and issubclass(training.BasicBlock, torch.nn.Module)


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "instance_stixels_core.h"
#define F(f) printf(#f " %zu %zu\n", offsetof(is_conv_bn_backward_args, f), sizeof(((is_conv_bn_backward_args*)0)->f));
int main() {
    printf(". %zu 0\n", sizeof(is_conv_bn_backward_args));
    FIELDS
    return 0;
}
"""


def test_args_layout_matches_the_header(tmp_path):
    cls = core.ConvBnBackwardArgs
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
# the device is touched).  2 frames of 32 -> 64 channels at 7 x 9: 63 cells, 4032 gradient elements per frame.
BIG = 1 << 40
F16, BF16, F32 = core.HEAD_F16, core.HEAD_BF16, core.HEAD_F32
GOOD = dict(d_features=0x100000, dtype=F16, n_images=2, channels_in=32, channels_out=64, rows8=7, cols8=9, kernel=3,
            dilation=2, d_weight=0x200000, d_scale=0x300000, d_out=0x400000, out_dtype=F16, relu=1,
            d_grad_out=0x500000, grad_out_dtype=F32, grad_image_stride=4032, d_grad_features=0x600000,
            grad_features_dtype=F16, d_grad_features_add=0x700000, d_grad_weight=0x800000, d_grad_scale=0x900000,
            d_grad_shift=0xa00000, d_grad_pre=0xb00000, d_scratch=0x10000000, scratch_bytes=BIG)
NEED = core.conv_bn_backward_scratch_bytes(2, 32, 64, 7, 9, 3, F16) if os.path.exists(core.LIB_PATH) else 0


@pytest.mark.parametrize("change, message", [
    # everything is_conv_bn refuses
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
    (dict(rows8=0), "rows8"),
    (dict(cols8=32768), "cols8"),
    (dict(dilation=0), "dilation"),
    (dict(dilation=9), "dilation"),
    (dict(kernel=1, dilation=2), "dilation must be 1"),
    (dict(relu=2), "relu"),
    (dict(out_dtype=BF16), "out_dtype"),
    # no output asked for
    (dict(d_grad_features=None, d_grad_features_add=None, d_grad_weight=None, d_grad_scale=None, d_grad_shift=None,
          d_grad_pre=None), "all null"),
    # dX with channels_in % 32
    (dict(channels_in=48), "channels_in % 32"),
    (dict(d_grad_features=None), "d_grad_features_add without"),
    (dict(grad_out_dtype=BF16), "grad_out_dtype"),
    (dict(grad_features_dtype=BF16), "grad_features_dtype"),
    (dict(grad_image_stride=4031), "grad_image_stride"),
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
    (dict(d_scale=0x300002), "aligned"),
    (dict(d_grad_weight=0x800002), "aligned"),
    (dict(d_grad_scale=0x900002), "aligned"),
    (dict(d_grad_shift=0xa00002), "aligned"),
    # output bytes that overlap inputs or each other (2 * 32 * 63 * 2 = 8064 bytes of features)
    (dict(d_grad_features=0x100000 + 8062), "overlap an input"),
    (dict(d_grad_pre=0x400000), "overlap an input"),
    (dict(d_grad_pre=0x500000 + 2 * 4032 * 4 - 2), "overlap an input"),
    (dict(d_grad_weight=0x200000 + 64 * 32 * 9 * 4 - 4), "overlap an input"),
    (dict(d_grad_shift=0x300000 + 252), "overlap an input"),
    (dict(d_grad_features=0x700000), "overlap an input"),
    (dict(d_grad_scale=0xa00000 - 252), "two outputs"),
    (dict(d_grad_pre=0x600000 + 8062), "two outputs"),
    (dict(d_scratch=0x100000), "overlap"),
    (dict(d_scratch=0x800000), "overlap"),
    # scratch
    (dict(d_scratch=None), "null d_scratch"),
    (dict(d_scratch=0x10000008), "16-byte"),
    (dict(scratch_bytes=NEED - 1), "scratch_bytes"),
    # last
    (dict(reserved=(0, 0, 1, 0)), "reserved"),
])
def test_refusals_need_no_device(change, message):
    rc = core.conv_bn_backward_ptr(**dict(GOOD, **change))
    assert rc == -1                                                          # IS_EINVAL
    assert re.search(message, core.lib().is_last_error().decode()), core.lib().is_last_error()


def test_reserved_is_the_last_refusal_and_null_args():
    # a call that is refused for the reserved field alone has passed every other check: the same call with another
    # fault names that fault
    assert core.conv_bn_backward_ptr(**dict(GOOD, reserved=(1, 0, 0, 0), d_scratch=0x10000008)) == -1
    assert b"16-byte" in core.lib().is_last_error()
    assert core.lib().is_conv_bn_backward(None, None) == -1
    assert b"null args" in core.lib().is_last_error()
    # the saved output is not looked at without relu
    assert core.conv_bn_backward_ptr(**dict(GOOD, relu=0, d_out=None, out_dtype=9, reserved=(1, 0, 0, 0))) == -1
    assert b"reserved" in core.lib().is_last_error()


def test_scratch_bytes():
    sb = core.conv_bn_backward_scratch_bytes
    for bad in ((0, 32, 64, 7, 9, 3, F16), (65536, 32, 64, 7, 9, 3, F16), (1, 24, 64, 7, 9, 3, F16),
                (1, 32, 48, 7, 9, 3, F16), (1, 32, 64, 0, 9, 3, F16), (1, 32, 64, 7, 32768, 3, F16),
                (1, 32, 64, 7, 9, 2, F16), (1, 32, 64, 7, 9, 3, F32), (65535, 2048, 2048, 32767, 9, 3, F16)):
        assert sb(*bad) == 0, bad
    al = lambda b: (b + 15) // 16 * 16
    B = core.CONV_BACKWARD_BAND

    def want(n, cin, cout, H, W, k):
        taps, P = k * k, H * W
        return (al(n * cout * P * 2) + al(cin * cout * taps * 2) + 2 * al(cin * 4) + al(n * cout * ((P + 2047) // 2048) * 8)
                + al(cout * cin * taps * 8) + al(n * ((H + B - 1) // B) * taps * cout * cin * 4))

    for shape in ((2, 32, 64, 7, 9, 3), (3, 48, 32, 2 * B + 5, 33, 1), (1, 512, 512, 16, 32, 3)):
        assert sb(*shape, F16) == sb(*shape, BF16) == want(*shape), shape


@pytest.mark.parametrize("kernel", cbr.KERNELS)
@pytest.mark.parametrize("s", [1, 5, 8, 9], ids=lambda s: cbr.SHAPE_IDS[s])
@pytest.mark.parametrize("relu, with_res", [(True, True), (True, False), (False, True)])
def test_reference_equals_float64_autograd_on_exact_inputs(s, kernel, relu, with_res):
    """On the exact family the half rounding changes no operand, scale is a power of two (so round_half(scale * w) is
    the product) and every sum is exact: the reference must BE float64 autograd of relu(scale conv(x, w) + shift +
    res), and the chain from (dscale, dshift) to bn.weight / bn.bias is the fold's derivative."""
    c, d = cbr.exact_inputs(s, kernel), cbr.dilation_of(s, kernel)
    w = c["m"] / 256.0
    res = c["res"] if with_res else None
    ag = cbr.autograd64(c["x"], w, c["scale"], c["shift"], res, c["dy"], kernel, d, relu=relu)
    for dtype in cbr.DTYPES:
        out_half = torch.from_numpy(ag["out"]).to(cbr.DTYPES[dtype])
        # (multiples of 2^-9: the rounding of the stored out moves no value onto 0, so its mask is the ReLU's)
        assert torch.equal(out_half.double() > 0, torch.from_numpy(ag["out"]) > 0)
        gh = cbr.masked_gradient(c["dy"], out_half, relu, dtype)
        if with_res:
            assert np.array_equal(gh.double().numpy(), ag["dres"])              # gh IS the residual's gradient
        r = cbr.backward(c["x"], c["w"], c["scale"], gh, kernel, d, dtype)
        for name in ("dx", "dw", "dscale", "dshift"):
            assert np.array_equal(r[name], ag[name]), (name, dtype)
    # the fold in the graph: scale = weight / sqrt(var + eps), shift = bias - mean * scale
    cout = c["scale"].size
    rng = np.random.default_rng(s)
    bn = (rng.standard_normal(cout), rng.standard_normal(cout), rng.standard_normal(cout), rng.uniform(0.5, 2.0, cout), 1e-5)
    ab = cbr.autograd64(c["x"], w, None, None, res, c["dy"], kernel, d, relu=relu, bn=bn)
    inv = 1.0 / np.sqrt(bn[3] + bn[4])
    assert np.allclose(ab["dbn_bias"], ab["dshift"], rtol=0, atol=0)
    assert np.allclose(ab["dbn_weight"], (ab["dscale"] - ab["dshift"] * bn[2]) * inv, rtol=1e-12, atol=1e-9)


def test_the_training_fold_reaches_weight_and_bias_as_the_reference_chain():
    bn = torch.nn.BatchNorm2d(8).eval()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(8)), bn.bias.copy_(torch.randn(8))
        bn.running_mean.copy_(torch.randn(8)), bn.running_var.copy_(torch.rand(8) + 0.5)
    f = training._FrozenBatchNorm(bn)
    scale, shift = f.fold()
    from instance_stixels_amd import cnn
    want = cnn.fold_batchnorm(bn)
    assert torch.equal(scale.detach(), want[0]) and torch.equal(shift.detach(), want[1])       # value for value
    gs, gb = torch.randn(8), torch.randn(8)
    torch.autograd.backward([scale, shift], [gs, gb])
    inv = 1.0 / torch.sqrt(bn.running_var.double() + bn.eps)
    assert torch.allclose(f.bias.grad.double(), gb.double(), rtol=1e-6, atol=0)
    assert torch.allclose(f.weight.grad.double(), (gs.double() - gb.double() * bn.running_mean.double()) * inv, rtol=1e-5,
                          atol=1e-6)
    f.train()
    before = f.running_mean.clone()
    f.fold()
    assert torch.equal(f.running_mean, before) and not f.running_mean.requires_grad


@pytest.mark.parametrize("kernel", cbr.KERNELS)
@pytest.mark.parametrize("s", range(len(cbr.SHAPES)), ids=cbr.SHAPE_IDS)
def test_the_exact_family_is_exact_in_both_dtypes(s, kernel):
    c = cbr.exact_inputs(s, kernel)
    n, cin, cout, H, W, d = cbr.SHAPES[s]
    for dtype in cbr.DTYPES:
        td = cbr.DTYPES[dtype]
        for name in ("x", "dy", "add", "res"):
            assert torch.equal(torch.from_numpy(c[name].copy()).to(td).float(), torch.from_numpy(c[name].copy())), name
        assert np.array_equal(torch.from_numpy(c["w"].copy()).to(td).double().numpy(), c["m"] / 256.0)
        ws = cbr.scaled_weight(c["w"], c["scale"], dtype).numpy()
        assert np.array_equal(ws, c["scale"].astype(np.float64).reshape(-1, 1, 1, 1) * c["m"] / 256.0)
    # every chunk sum stays below 2^24: at most min(BAND, H) * W products of at most 3 * 2 in magnitude
    assert min(cbr.BAND, H) * W * 6 < 2 ** 24
    # dX: at most taps * channels_out products of at most 2 * 2, multiples of 2^-9, plus the add of at most 8
    assert (kernel * kernel * cout * 4 + 8) * 2 ** 9 < 2 ** 24
    # dscale: multiples of 2^-8 below 2^53 in binary64
    assert cin * kernel * kernel * n * H * W * 6 * 2 ** 8 < 2 ** 53


def test_masked_gradient_reads_the_stored_output():
    dy = np.array([1.0, -2.0, 3.0, -0.0, 1e-9], np.float32)
    out = np.array([0.5, 0.0, -0.0, 1.0, 2.0], np.float32)
    for dtype in cbr.DTYPES:
        gh = cbr.masked_gradient(dy, out, True, dtype)
        assert gh.float().tolist()[:3] == [1.0, 0.0, 0.0]
        bits = gh.view(torch.int16).tolist()
        assert bits[1] == 0 and bits[2] == 0 and bits[3] == -32768          # +0 where inactive; an active -0 stays
        assert torch.equal(cbr.masked_gradient(dy, None, False, dtype), torch.from_numpy(dy).to(cbr.DTYPES[dtype]))


def _pair(stride=1, k=3, train=False):
    conv = torch.nn.Conv2d(32, 32, k, stride=stride, padding=k // 2, bias=False)
    bn = torch.nn.BatchNorm2d(32)
    return conv, (bn.train() if train else bn.eval())


def test_the_modules_refuse_what_they_do_not_cover():
    import conv_bn_reference as cb
    with pytest.raises(core.CoreError, match="stride"):
        training.ConvBnReLU(*_pair(stride=2))
    with pytest.raises(core.CoreError, match="batch statistics"):
        training.ConvBnReLU(*_pair(train=True))
    with pytest.raises(core.CoreError, match="running statistics"):
        training.ConvBnReLU(_pair()[0], torch.nn.BatchNorm2d(32, track_running_stats=False).eval())
    layer = training.ConvBnReLU(*_pair())
    assert {n for n, _ in layer.named_parameters()} == {"weight", "bn.weight", "bn.bias"}
    assert {n for n, _ in layer.named_buffers()} == {"bn.running_mean", "bn.running_var"}
    with pytest.raises(core.CoreError, match="fp32 features"):
        layer(torch.zeros(1, 32, 4, 4))
    with pytest.raises(core.CoreError, match="stride"):
        training.BasicBlock(cb.Block(32, 64, downsample=True, stride=2).eval())
    with pytest.raises(core.CoreError, match="batch statistics"):
        training.BasicBlock(cb.Block(32, 64, downsample=True).train())
    with pytest.raises(core.CoreError, match="Bottleneck"):
        b = cb.Block(32, 32).eval()
        b.conv3 = b.conv2
        training.BasicBlock(b)
    block = training.BasicBlock(cb.Block(32, 64, downsample=True).eval())
    assert len(list(block.parameters())) == 9
    with pytest.raises(core.CoreError, match="fp32 features"):
        block(torch.zeros(1, 32, 4, 4))
    with pytest.raises(core.CoreError, match="device tensor"):
        core.conv_bn_backward(torch.zeros(1, 32, 4, 4), None, None, None, None, 3)
