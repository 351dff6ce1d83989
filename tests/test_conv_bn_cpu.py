"""The residual blocks' launches (f18) without a GPU: the symbols and bindings, the struct layout, the ranges of
is_conv_packed_bytes, the refusals of is_conv_bn and is_conv_pack_weights (all made before the device is touched), the
refusals of cnn.ResidualBlock (made before anything is packed), and the reference of tests/conv_bn_reference.py pinned
against BasicBlock-shaped torch modules, against the claim that its exact inputs are exact, and against three wrong
epilogues that its bound has to catch; the signatures of the Python surface of f17 and f18, and the packers' refusals
(made before a device is touched)."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import conv3x3_reference as cr
import conv_bn_reference as cb
from instance_stixels_amd import cnn, core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("is_conv_packed_bytes", "is_conv_pack_weights", "is_conv_bn")


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "instance_stixels_core.h")).read()
    for name in NAMES:
        assert name + "(" in header, name
        assert name in core.EXPORTS and hasattr(core.lib(), name), name
    for fn in ("conv_packed_bytes", "conv_pack_weights", "conv_bn", "conv_bn_ptr"):
        assert callable(getattr(core, fn)), fn
    assert callable(cnn.ResidualBlock) and callable(cnn.DrnDilated)
    for cite in ("drn.py:54-87", "drn.py:168-172", "drn.py:199-221"):
        assert cite in header, cite
    # the contract stands in the header and in the kernel's top comment: the residual epilogue and the 1x1 form
    kernel = open(os.path.join(ROOT, "instance_stixels_amd", "csrc", "is_k_conv3x3.hip")).read()
    for text in (header, kernel):
        assert "fmaf(scale[co], a, shift[co])" in text and "(float)residual[n][co][y][x]" in text
        assert "two fp32 roundings" in text or "two roundings" in text
        assert "1x1" in text
    assert "HALF tensors under amp" in header and "single final rounding" in header


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "instance_stixels_core.h"
#define F(f) printf(#f " %zu %zu\n", offsetof(is_conv_bn_args, f), sizeof(((is_conv_bn_args*)0)->f));
int main() {
    printf(". %zu 0\n", sizeof(is_conv_bn_args));
    FIELDS
    return 0;
}
"""


def test_args_layout_matches_the_header(tmp_path):
    src = PROBE.replace("FIELDS", "".join(f"F({n})" for n, _ in core.ConvBnArgs._fields_))
    (tmp_path / "probe.cpp").write_text(src)
    exe = str(tmp_path / "probe")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "probe.cpp"), "-o", exe],
                   check=True)
    got = {f: (int(off), int(size)) for f, off, size in
           (l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())}
    assert got["."][0] == ctypes.sizeof(core.ConvBnArgs) == 112
    declared = re.search(r"typedef struct is_conv_bn_args \{(.*?)\} is_conv_bn_args;",
                         open(os.path.join(ROOT, "include", "instance_stixels_core.h")).read(), re.S).group(1)
    declared = re.sub(r"/\*.*?\*/", "", declared, flags=re.S)
    names = re.findall(r"(\w+)(?:\[4\])?\s*[,;]", declared)
    assert names == [n for n, _ in core.ConvBnArgs._fields_]
    for name, _ in core.ConvBnArgs._fields_:
        field = getattr(core.ConvBnArgs, name)
        assert got[name] == (field.offset, field.size), name
    # f17's struct is a prefix-compatible subset by name: every field of it exists here
    assert {n for n, _ in core.Conv3x3Args._fields_} <= {n for n, _ in core.ConvBnArgs._fields_}


def test_packed_bytes_honours_the_ranges():
    pb = core.conv_packed_bytes
    for dt in (core.HEAD_F16, core.HEAD_BF16):
        for k in (1, 3):
            for cout, cin in ((32, 16), (512, 512), (2048, 2048), (64, 48), (256, 128)):
                assert pb(cout, cin, k, dt) == cout * cin * k * k * 2
            for cout, cin in ((0, 16), (16, 16), (48, 16), (2080, 16), (32, 0), (32, 8), (32, 24), (32, 2064), (-32, 16),
                              (32, -16)):
                assert pb(cout, cin, k, dt) == 0, (cout, cin, k)
        for k in (0, 2, 5, -1, 9):
            assert pb(32, 16, k, dt) == 0, k
        assert pb(64, 48, 3, dt) == core.conv3x3_packed_bytes(64, 48, dt)
    for dt in (core.HEAD_F32, 3, -1):
        assert pb(32, 16, 3, dt) == 0 and pb(32, 16, 1, dt) == 0


# A call that would be accepted (the pointers are never dereferenced on the host: every case below is refused before
# the device is touched).  Features 1*16*5*7 bf16 = 1120 B at 0x10000, output 1*32*5*7 bf16 = 2240 B at 0x20000,
# residual 2240 B at 0x60000.
GOOD = dict(d_features=0x10000, dtype=core.HEAD_BF16, n_images=1, channels_in=16, channels_out=32, rows8=5, cols8=7,
            kernel=3, dilation=2, d_packed=0x30000, d_scale=0x40000, d_shift=0x50000, d_residual=0x60000, relu=1,
            d_out=0x20000, out_dtype=core.HEAD_BF16)


@pytest.mark.parametrize("change, message", [
    # f17's
    (dict(d_features=None), "null"),
    (dict(d_packed=None), "null"),
    (dict(d_scale=None), "null"),
    (dict(d_shift=None), "null"),
    (dict(d_out=None), "null"),
    (dict(dtype=core.HEAD_F32, out_dtype=core.HEAD_F32), "dtype"),
    (dict(dtype=3), "dtype"),
    (dict(dtype=-1), "dtype"),
    (dict(out_dtype=core.HEAD_F16), "out_dtype"),
    (dict(out_dtype=7), "out_dtype"),
    (dict(channels_in=0), "channels_in"),
    (dict(channels_in=24), "channels_in"),
    (dict(channels_in=2064), "channels_in"),
    (dict(channels_out=16), "channels_out"),
    (dict(channels_out=48), "channels_out"),
    (dict(channels_out=2080), "channels_out"),
    (dict(dilation=0), "dilation"),
    (dict(dilation=9), "dilation"),
    (dict(rows8=0), "rows8"),
    (dict(rows8=32768), "rows8"),
    (dict(cols8=0), "cols8"),
    (dict(cols8=32768), "cols8"),
    (dict(n_images=0), "n_images"),
    (dict(n_images=65536), "n_images"),
    (dict(relu=2), "relu"),
    (dict(relu=-1), "relu"),
    (dict(d_packed=0x30008), "d_packed must be 16-byte aligned"),
    (dict(d_features=0x10001), "d_features must be aligned"),
    (dict(d_out=0x20002, out_dtype=core.HEAD_F32), "d_out must be aligned"),
    (dict(d_out=0x10000), "d_out overlaps d_features"),
    (dict(d_out=0x10000 + 1118), "d_out overlaps d_features"),
    (dict(d_out=0x10000 - 2240 + 2), "d_out overlaps d_features"),
    (dict(kernel=1, dilation=1, d_out=0x10000), "d_out overlaps d_features"),
    (dict(reserved=(0, 0, 1, 0)), "reserved"),
    (dict(reserved=(0, 0, 0, -1), d_residual=None), "reserved"),
    # f18's
    (dict(kernel=0), "kernel"),
    (dict(kernel=2), "kernel"),
    (dict(kernel=5), "kernel"),
    (dict(kernel=9), "kernel"),
    (dict(kernel=1, dilation=2), "dilation must be 1 with kernel 1"),
    (dict(kernel=1, dilation=0), "dilation must be 1 with kernel 1"),
    (dict(d_residual=0x60001), "d_residual must be aligned"),
    (dict(d_residual=0x20000), "d_out overlaps d_residual"),                 # the output itself
    (dict(d_residual=0x20000 + 2238), "d_out overlaps d_residual"),          # the output's last element
    (dict(d_residual=0x20000 - 2240 + 2), "d_out overlaps d_residual"),      # the output's first element
    (dict(d_residual=0x20000 + 4480 - 2, out_dtype=core.HEAD_F32), "d_out overlaps d_residual"),   # fp32: 4480 B
])
def test_refusals_need_no_device(change, message):
    rc = core.conv_bn_ptr(**dict(GOOD, **change))
    assert rc == -1                                                          # IS_EINVAL
    assert re.search(message, core.lib().is_last_error().decode()), core.lib().is_last_error()


def test_residual_may_be_the_features_and_may_touch_the_output():
    """A call accepted up to the device cannot be run here.  The reserved fields are checked last, so a call refused
    for them alone has passed every check of the residual: the features as residual (channels_in = channels_out), a
    residual ending where the output begins, one beginning where it ends, and none at all."""
    same = dict(GOOD, channels_in=32, d_residual=GOOD["d_features"])
    for call in (same, dict(same, kernel=1, dilation=1), dict(GOOD, d_residual=0x20000 - 2240),
                 dict(GOOD, d_residual=0x20000 + 2240), dict(GOOD, d_residual=None)):
        assert core.conv_bn_ptr(**dict(call, reserved=(1, 0, 0, 0))) == -1
        message = core.lib().is_last_error().decode()
        assert "reserved" in message and "residual" not in message and "overlap" not in message, message
    # and with another field wrong in the same call, the refusal names that field
    assert core.conv_bn_ptr(**dict(same, relu=2)) == -1
    message = core.lib().is_last_error().decode()
    assert "relu" in message and "residual" not in message, message


def test_null_args_and_pack_refusals():
    L = core.lib()
    assert L.is_conv_bn(None, None) == -1
    assert b"null args" in L.is_last_error()
    for args, message in (((None, 32, 16, 3, core.HEAD_F16, 0x1000), b"null"),
                          ((0x1000, 32, 16, 1, core.HEAD_F16, None), b"null"),
                          ((0x1000, 32, 16, 3, core.HEAD_F32, 0x2000), b"dtype"),
                          ((0x1000, 48, 16, 1, core.HEAD_F16, 0x2000), b"channels_out"),
                          ((0x1000, 32, 8, 1, core.HEAD_F16, 0x2000), b"channels_in"),
                          ((0x1000, 32, 16, 2, core.HEAD_F16, 0x2000), b"kernel"),
                          ((0x1000, 32, 16, 0, core.HEAD_BF16, 0x2000), b"kernel"),
                          ((0x1002, 32, 16, 1, core.HEAD_F16, 0x2000), b"d_weight"),
                          ((0x1000, 32, 16, 1, core.HEAD_F16, 0x2004), b"d_packed")):
        assert L.is_conv_pack_weights(*args, None) == -1, args
        assert message in L.is_last_error(), (args, L.is_last_error())


# ---- BasicBlock-shaped modules ----

Block, _bn = cb.Block, cb.batchnorm


def _fold64(bn):
    scale = (bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)).detach()
    return scale.numpy(), (bn.bias.double() - bn.running_mean.double() * scale).detach().numpy()


@pytest.mark.parametrize("form", ["downsample", "identity", "no_residual"])
def test_reference_is_the_basic_block_of_the_reference_model(form):
    """The block in float64 and eval mode against three (two) calls of the reference with unrounded operands
    (dtype None) and the float64 fold."""
    cin, cout = (16, 32) if form == "downsample" else (32, 32)
    block = Block(cin, cout, dilation=(2, 4), downsample=form == "downsample", residual=form != "no_residual",
                  seed=20).double().eval()
    x = torch.randn(2, cin, 9, 11, generator=torch.Generator().manual_seed(21)).double()
    with torch.no_grad():
        want = block(x)
    w1, w2 = block.conv1.weight.detach().numpy(), block.conv2.weight.detach().numpy()
    y = cb.reference(x.numpy(), w1, *_fold64(block.bn1), 3, 2, None)["ref"]
    res = None
    if form == "downsample":
        res = cb.reference(x.numpy(), block.downsample[0].weight.detach().numpy(), *_fold64(block.downsample[1]), 1, 1,
                           None, relu=False)["ref"]
        assert (res < 0).any()
    elif form == "identity":
        res = x.numpy()
    got = cb.reference(y, w2, *_fold64(block.bn2), 3, 4, None, residual=res)
    assert np.allclose(got["ref"], want.numpy(), rtol=1e-12, atol=1e-12)
    assert (want > 0).any() and (want == 0).any()
    if res is not None:          # the residual decides the sign of some elements, and the epilogue's steps are kept
        assert (np.sign(got["pre"]) != np.sign(got["prerelu"])).any()
        assert np.array_equal(got["prerelu"], got["pre"] + res)
    else:
        assert np.array_equal(got["prerelu"], got["pre"])
    assert np.array_equal(got["ref"], np.maximum(got["prerelu"], 0.0))


def test_reference_without_residual_is_f17s():
    s = 1
    n, cin, cout, H, W, d = cb.SHAPES[s]
    assert cb.SHAPES[:5] == cr.SHAPES[:5]
    c = cr.random_inputs(s)
    for dtype in sorted(cb.DTYPES):
        old = cr.random_reference(s, dtype)
        new = cb.reference(c["x"], c["w"], c["scale"], c["shift"], 3, d, dtype)
        assert np.array_equal(new["ref"], old["ref"])
        # f17 takes the ulp at the value after the ReLU, f18 at the value before it: never smaller
        assert (new["tol"] >= old["tol"]).all()


CASES = [(s, k) for s in range(len(cb.SHAPES)) for k in cb.KERNELS]
CASE_IDS = ["%s-k%d" % (cb.SHAPE_IDS[s], k) for s, k in CASES]


@pytest.mark.parametrize("dtype", sorted(cb.DTYPES))
@pytest.mark.parametrize("s, kernel", CASES, ids=CASE_IDS)
def test_exact_inputs_are_exact(s, kernel, dtype):
    """Both half dtypes hold the features and the residual as given and round the weights back to m / 256; every
    value of the float64 reference, before and after each step of the epilogue, is a multiple of 2^-9 below 2^15 and
    an fp32 value."""
    c = cb.exact_inputs(s, kernel)
    for name in ("x", "res"):
        assert torch.equal(cr.round_half(c[name], dtype), torch.from_numpy(c[name].astype(np.float64)))
    assert np.abs(c["res"]).max() == 8 and c["x"].max() == 3 and c["x"].min() == 0
    assert torch.equal(cr.round_half(c["w"], dtype), torch.from_numpy(c["m"] / 256.0))
    assert not np.array_equal(c["w"].astype(np.float64), c["m"] / 256.0)      # (the pack call has to round)
    assert set(np.abs(c["scale"]).tolist()) <= {0.5, 1.0, 2.0} and (c["scale"] < 0).any() and (c["scale"] > 0).any()
    assert np.array_equal(c["shift"], np.round(c["shift"])) and np.abs(c["shift"]).max() <= 4
    for with_res in (False, True):
        for relu in (True, False):
            r = cb.exact_reference(s, kernel, with_res, relu)
            assert r["A"].max() < 2.0 ** 14
            for name in ("ref", "pre", "prerelu"):
                assert np.abs(r[name]).max() < 2.0 ** 15
                assert np.array_equal(r[name] * 512.0, np.round(r[name] * 512.0))
                assert np.array_equal(r[name].astype(np.float32).astype(np.float64), r[name])
    if s < 4:                    # the same reference from the generic path on the rounded operands
        g = cb.reference(c["x"], c["w"], c["scale"], c["shift"], kernel, cb.dilation_of(s, kernel), dtype,
                         residual=c["res"])
        assert np.array_equal(g["ref"], cb.exact_reference(s, kernel, True)["ref"])


def _contract_fp32(c, dtype, kernel, d, residual, relu=True, wrong=None):
    """The contract evaluated in fp32 on the CPU (torch's convolution in fp32, then the epilogue step by step in
    numpy fp32), or one of three wrong versions of it."""
    x32, w32 = cr.round_half(c["x"], dtype).float(), cr.round_half(c["w"], dtype).float()
    if wrong == "dropped_term":
        w32 = w32.clone()
        w32[0, 0, kernel // 2, kernel // 2] = 0.0
    a = torch.nn.functional.conv2d(x32, w32, padding=d if kernel == 3 else 0, dilation=d).numpy()
    v = (c["scale"].reshape(1, -1, 1, 1) * a + c["shift"].reshape(1, -1, 1, 1)).astype(np.float32)
    if residual is not None:
        res = cr.round_half(residual, dtype).float().numpy()
        if wrong == "wrong_channel":
            res = np.roll(res, 1, axis=1)
        if wrong == "after_relu":
            return (np.maximum(v, np.float32(0)) + res).astype(np.float32)
        v = (v + res).astype(np.float32)
    return np.maximum(v, np.float32(0)) if relu else v


@pytest.mark.parametrize("kernel", cb.KERNELS)
def test_bound_catches_wrong_epilogues_and_passes_fp32(kernel):
    """At (16, 32, 5x7): an fp32 evaluation of the contract stays far inside the bound; a dropped term, a residual
    taken from the neighbouring channel and a residual added after the ReLU are far outside it."""
    s = 0
    d = cb.dilation_of(s, kernel)
    c = cb.random_inputs(s, kernel)
    for dtype in sorted(cb.DTYPES):
        for with_res in (False, True):
            r = cb.random_reference(s, kernel, dtype, with_res)
            res = c["res"] if with_res else None
            ratio = np.abs(_contract_fp32(c, dtype, kernel, d, res).astype(np.float64) - r["ref"]) / r["tol"]
            assert ratio.max() < 0.2, ratio.max()
            wrongs = ("dropped_term", "wrong_channel", "after_relu") if with_res else ("dropped_term",)
            for wrong in wrongs:
                bad = np.abs(_contract_fp32(c, dtype, kernel, d, res, wrong=wrong).astype(np.float64) - r["ref"]) / r["tol"]
                assert bad.max() > 10, (wrong, bad.max())
        r0 = cb.random_reference(s, kernel, dtype, True, relu=False)
        ratio = np.abs(_contract_fp32(c, dtype, kernel, d, c["res"], relu=False).astype(np.float64) - r0["ref"]) / r0["tol"]
        assert ratio.max() < 0.2 and (r0["ref"] < 0).any()


# ---- cnn.ResidualBlock: every refusal is made before anything is packed, so none needs a device ----

class _Bottleneck(Block):
    def __init__(self):
        super().__init__(32, 32)
        self.conv3 = torch.nn.Conv2d(32, 32, 1, bias=False)


@pytest.mark.parametrize("make, message", [
    (lambda: Block(32, 32, stride=2, downsample=True).eval(), "stride"),
    (lambda: _strided_downsample(), "downsample has stride"),
    (lambda: _Bottleneck().eval(), "Bottleneck"),
    (lambda: Block(32, 32).train(), "eval"),
    (lambda: _training_downsample(), "eval"),
    (lambda: _with_downsample(torch.nn.Sequential(torch.nn.Conv2d(32, 64, 1, bias=True), _bn(64, 1))), "downsample must be"),
    (lambda: _with_downsample(torch.nn.Sequential(torch.nn.Conv2d(32, 64, 3, padding=1, bias=False), _bn(64, 1))), "downsample must be"),
    (lambda: _with_downsample(torch.nn.Sequential(torch.nn.Conv2d(32, 64, 1, bias=False))), "downsample must be"),
    (lambda: _with_downsample(torch.nn.Conv2d(32, 64, 1, bias=False)), "downsample must be"),
    (lambda: Block(32, 64, downsample=False, residual=True).eval(), "without a downsample"),
])
def test_residual_block_refusals_need_no_device(make, message):
    with pytest.raises(core.CoreError, match=message):
        cnn.ResidualBlock(make())


def _with_downsample(down):
    block = Block(32, 64, downsample=True).eval()
    block.downsample = down.eval()
    return block


# ---- the Python surface of f17 and f18: the signatures, and the packers' refusals ahead of the device ----

SIGNATURES = [
    (core.conv3x3_packed_bytes, "(channels_out, channels_in, dtype)"),
    (core.conv3x3_pack_weights, "(weight, dtype, device=0)"),
    (core.conv3x3_bn_relu_ptr, "(stream=0, **fields)"),
    (core.conv3x3_bn_relu, "(features, packed, scale, shift, dilation, relu=True, out_dtype=None, canary=0)"),
    (core.conv_packed_bytes, "(channels_out, channels_in, kernel, dtype)"),
    (core.conv_pack_weights, "(weight, dtype, device=0)"),
    (core.conv_bn_ptr, "(stream=0, **fields)"),
    (core.conv_bn, "(features, packed, scale, shift, kernel, dilation=1, residual=None, relu=True, out_dtype=None, "
                   "canary=0)"),
    (cnn.ConvBnRelu.__init__, "(self, conv, bn, dtype=torch.bfloat16, relu=True, device=0)"),
    (cnn.ResidualBlock.__init__, "(self, block, dtype=torch.bfloat16, device=0)"),
    (cnn.DrnTail.__init__, "(self, layer7, layer8, seg, n_classes, rows_power2_segmentation, clamp=None, "
                           "dtype=torch.bfloat16, device=0)"),
    (cnn.DrnDilated.__init__, "(self, layer5, layer6, layer7, layer8, seg, n_classes, rows_power2_segmentation, "
                              "clamp=None, dtype=torch.bfloat16, device=0)"),
]


@pytest.mark.parametrize("fn, signature", SIGNATURES, ids=[fn.__qualname__ for fn, _ in SIGNATURES])
def test_public_signatures_are_pinned(fn, signature):
    """Parameter names, order and defaults of the eight conv functions and of the four layer classes."""
    assert str(inspect.signature(fn)) == signature


@pytest.mark.parametrize("pack, weight, dtype, message", [
    (core.conv3x3_pack_weights, (32, 16, 5, 5), torch.bfloat16, r"\[channels_out\]\[channels_in\]\[3\]\[3\]"),
    (core.conv3x3_pack_weights, (32, 16, 3, 3), torch.float32, "neither torch.float16 nor torch.bfloat16"),
    # (a 5x5 weight is [k][k]: is_conv_packed_bytes, a host function, refuses its k)
    (core.conv_pack_weights, (32, 16, 5, 5), torch.bfloat16, "is_conv_packed_bytes refuses .* kernel 5"),
    (core.conv_pack_weights, (32, 16, 3, 5), torch.bfloat16, r"\[channels_out\]\[channels_in\]\[k\]\[k\]"),
    (core.conv_pack_weights, (32, 16, 3, 3), torch.float32, "neither torch.float16 nor torch.bfloat16"),
], ids=["f17-5x5", "f17-float32", "f18-5x5", "f18-3x5", "f18-float32"])
def test_pack_refusals_come_before_the_device(pack, weight, dtype, message, monkeypatch):
    """A CPU weight that a packer refuses is refused before it is copied to a device or a stream is asked for."""
    def touched(*args, **kwargs):
        raise AssertionError("the device was touched before the refusal")
    w = torch.zeros(weight)
    monkeypatch.setattr(torch.Tensor, "to", touched)
    monkeypatch.setattr(core, "_current_stream", touched)
    with pytest.raises(core.CoreError, match=message):
        pack(w, dtype)


def _strided_downsample():
    block = Block(32, 64, downsample=True).eval()
    block.downsample[0].stride = (2, 2)
    return block


def _training_downsample():
    block = Block(32, 64, downsample=True).eval()
    block.downsample[1].train()
    return block
