"""The downsampling layers' launches (f19) without a GPU: the symbols and bindings, the struct layout against a compiled
probe, the new refusals of is_conv_bn_stride (all made before the device is touched), the output extents, the reference
of tests/conv_stride_reference.py pinned against strided BasicBlock-shaped torch modules, against the claim that its
exact inputs are exact and against three wrong forms of a strided convolution that its bound has to catch, the refusals
of cnn.StridedResidualBlock (made before anything is packed), and the signatures of the new Python surface."""
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
import conv_stride_reference as cs
from instance_stixels_amd import cnn, core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "instance_stixels_core.h")
Block, _bn = cb.Block, cb.batchnorm


def test_symbols_are_declared_exported_and_bound():
    header = open(HEADER).read()
    assert "is_conv_bn_stride(" in header
    assert "is_conv_bn_stride" in core.EXPORTS and hasattr(core.lib(), "is_conv_bn_stride")
    for fn in ("conv_bn_stride", "conv_bn_stride_ptr"):
        assert callable(getattr(core, fn)), fn
    assert issubclass(core.ConvBnStrideArgs, ctypes.Structure)
    assert issubclass(cnn.StridedResidualBlock, cnn.ResidualBlock) and callable(cnn.DrnDownsampling)
    # the contract stands in the header and in the kernel's top comment: the layers, the output extent, the sampling,
    # and that stride 2 means dilation 1
    kernel = open(os.path.join(ROOT, "instance_stixels_amd", "csrc", "is_k_conv3x3.hip")).read()
    for text in (header, kernel):
        assert "drn.py:161-167" in text and "layer2" in text and "layer4" in text
        assert re.search(r"\(rows_in \+ 1\) / 2|\(H \+ 1\) / 2", text)
        assert re.search(r"\[2 ?y \+ ky - 1\]\[2 ?x \+ kx - 1\]", text) and re.search(r"\[2 ?y\]\[2 ?x\]", text)
        assert re.search(r"stride 2 means dilation 1|dilation 1 only", text)
    assert "floor((H + 2 p - d (k - 1) - 1) / 2) + 1" in header and "drn.py:199-221" in header


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "instance_stixels_core.h"
#define F(f) printf(#f " %zu %zu\n", offsetof(is_conv_bn_stride_args, f), sizeof(((is_conv_bn_stride_args*)0)->f));
int main() {
    printf(". %zu 0\n", sizeof(is_conv_bn_stride_args));
    printf("is_conv_bn_args %zu 0\n", sizeof(is_conv_bn_args));
    printf("is_conv3x3_args %zu 0\n", sizeof(is_conv3x3_args));
    FIELDS
    return 0;
}
"""


def test_args_layout_matches_the_header(tmp_path):
    fields = core.ConvBnStrideArgs._fields_
    (tmp_path / "probe.cpp").write_text(PROBE.replace("FIELDS", "".join(f"F({n})" for n, _ in fields)))
    exe = str(tmp_path / "probe")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "probe.cpp"), "-o", exe],
                   check=True)
    got = {f: (int(off), int(size)) for f, off, size in
           (l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())}
    assert got["."][0] == ctypes.sizeof(core.ConvBnStrideArgs)
    assert got["is_conv_bn_args"][0] == ctypes.sizeof(core.ConvBnArgs) == 112          # f18's struct did not grow
    assert got["is_conv3x3_args"][0] == ctypes.sizeof(core.Conv3x3Args) == 104         # nor f17's
    declared = re.search(r"typedef struct is_conv_bn_stride_args \{(.*?)\} is_conv_bn_stride_args;",
                         open(HEADER).read(), re.S).group(1)
    declared = re.sub(r"/\*.*?\*/", "", declared, flags=re.S)
    names = re.findall(r"(\w+)(?:\[4\])?\s*[,;]", declared)
    assert names == [n for n, _ in fields]
    for name, _ in fields:
        field = getattr(core.ConvBnStrideArgs, name)
        assert got[name] == (field.offset, field.size), name
    # is_conv_bn_args' fields with rows8 / cols8 renamed, plus the stride
    old = [{"rows8": "rows_in", "cols8": "cols_in"}.get(n, n) for n, _ in core.ConvBnArgs._fields_]
    assert [n for n, _ in fields if n != "stride"] == old and "rows8" not in dict(fields)


# A call that would be accepted (the pointers are never dereferenced on the host: every case below is refused before
# the device is touched).  Features 1*16*5*7 bf16 = 1120 B at 0x10000; at stride 2 the output is 1*32*3*4 bf16 = 768 B
# at 0x20000 and the residual 768 B at 0x60000.
GOOD = dict(d_features=0x10000, dtype=core.HEAD_BF16, n_images=1, channels_in=16, channels_out=32, rows_in=5, cols_in=7,
            kernel=3, stride=2, dilation=1, d_packed=0x30000, d_scale=0x40000, d_shift=0x50000, d_residual=0x60000,
            relu=1, d_out=0x20000, out_dtype=core.HEAD_BF16)
RESERVED = dict(reserved=(0, 1, 0, 0))


def _refused(call):
    assert core.conv_bn_stride_ptr(**call) == -1                               # IS_EINVAL
    return core.lib().is_last_error().decode()


@pytest.mark.parametrize("change, message", [
    # the new refusals
    (dict(stride=0), "stride is neither 1 nor 2"),
    (dict(stride=3), "stride is neither 1 nor 2"),
    (dict(stride=-2), "stride is neither 1 nor 2"),
    (dict(stride=4), "stride is neither 1 nor 2"),
    (dict(dilation=2), "dilation must be 1 with stride 2"),
    (dict(dilation=8), "dilation must be 1 with stride 2"),
    (dict(channels_in=32, d_residual=0x10000), "d_residual is d_features with stride 2"),
    (dict(kernel=1, channels_in=32, d_residual=0x10000), "d_residual is d_features with stride 2"),
    # every buffer at its own size: the output and the residual are 768 B, the features 1120 B
    (dict(d_out=0x10000 + 1118), "d_out overlaps d_features"),                 # the features' last element
    (dict(d_out=0x10000 - 768 + 2), "d_out overlaps d_features"),              # the output's last on their first
    (dict(d_residual=0x20000 + 766), "d_out overlaps d_residual"),
    (dict(d_residual=0x20000 - 768 + 2), "d_out overlaps d_residual"),
    (dict(d_residual=0x20000 + 1536 - 2, out_dtype=core.HEAD_F32), "d_out overlaps d_residual"),   # fp32: 1536 B
    # is_conv_bn's, through this entry; the extents under their names here
    (dict(rows_in=0), "rows_in"),
    (dict(cols_in=32768), "cols_in"),
    (dict(d_features=None), "null"),
    (dict(kernel=2), "kernel"),
    (dict(kernel=1, stride=1, dilation=2), "dilation must be 1 with kernel 1"),
    (dict(stride=1, dilation=9), r"dilation outside \[1, 8\]"),
    (dict(channels_out=48), "channels_out"),
    (dict(relu=2), "relu"),
    (dict(d_residual=0x60001), "d_residual must be aligned"),
    (RESERVED, "reserved"),
    (dict(reserved=(0, 0, 0, -1), d_residual=None), "reserved"),
])
def test_refusals_need_no_device(change, message):
    assert re.search(message, _refused(dict(GOOD, **change)))


def test_calls_refused_for_reserved_alone_have_passed_every_other_check():
    """A call accepted up to the device cannot be run here.  The reserved fields are checked last, so a call refused
    for them alone has passed every other check: buffers that touch at each one's OWN size (with the features' size for
    the output, or the input's extents for the residual, these would not be refused, or would be refused for overlap),
    stride 1 with every dilation and with the features as residual, no residual."""
    calls = [
        GOOD, dict(GOOD, kernel=1), dict(GOOD, d_residual=None),
        dict(GOOD, d_out=0x10000 + 1120), dict(GOOD, d_out=0x10000 - 768),          # the output touches the features
        dict(GOOD, d_residual=0x20000 + 768), dict(GOOD, d_residual=0x20000 - 768),  # the residual touches the output
        dict(GOOD, d_residual=0x20000 + 1536, out_dtype=core.HEAD_F32),
        dict(GOOD, d_residual=0x10000 + 2),                                          # the residual inside the features
        dict(GOOD, stride=1, dilation=8, d_residual=None),
        dict(GOOD, stride=1, channels_in=32, d_residual=0x10000),                    # stride 1: residual == features
        dict(GOOD, stride=1, kernel=1, channels_in=32, d_residual=0x10000),
        dict(GOOD, rows_in=32767, cols_in=32767, n_images=1, d_out=0x7f0000000000, d_residual=None),
    ]
    for call in calls:
        message = _refused(dict(call, **RESERVED))
        assert "reserved" in message and "overlap" not in message and "stride" not in message, (call, message)
    # ... and the same buffers one element closer are refused for their overlap
    assert "d_out overlaps d_features" in _refused(dict(GOOD, d_out=0x10000 + 1118, **RESERVED))
    assert "d_out overlaps d_residual" in _refused(dict(GOOD, d_residual=0x20000 + 766, **RESERVED))
    # stride 1 takes the input's extents for all three: 32 * 5 * 7 * 2 = 2240 B of output
    assert "d_out overlaps d_residual" in _refused(dict(GOOD, stride=1, d_residual=0x20000 + 2238))
    assert "reserved" in _refused(dict(GOOD, stride=1, d_residual=0x20000 + 2240, **RESERVED))


def test_null_args_and_the_old_entry_points_keep_their_words():
    L = core.lib()
    assert L.is_conv_bn_stride(None, None) == -1
    assert b"null args" in L.is_last_error()
    old = {k: v for k, v in GOOD.items() if k not in ("rows_in", "cols_in", "stride")}
    assert core.conv_bn_ptr(**dict(old, rows8=0, cols8=7)) == -1
    assert b"rows8 and cols8" in L.is_last_error() and b"rows_in" not in L.is_last_error()
    assert core.conv_bn_stride_ptr(**dict(GOOD, rows_in=0)) == -1
    assert b"rows_in and cols_in" in L.is_last_error() and b"rows8" not in L.is_last_error()
    # is_conv_bn is the stride-1 call: its reserved fields stay refused, and it cannot be given a stride
    assert core.conv_bn_ptr(**dict(old, rows8=5, cols8=7, reserved=(2, 0, 0, 0))) == -1
    assert b"reserved" in L.is_last_error()
    assert "stride" not in dict(core.ConvBnArgs._fields_)


KERNEL_CASES = [(s, k) for s in range(len(cs.SHAPES)) for k in cs.KERNELS]
KERNEL_IDS = ["%s-k%d" % (cs.SHAPE_IDS[s], k) for s, k in KERNEL_CASES]


@pytest.mark.parametrize("s, kernel", KERNEL_CASES, ids=KERNEL_IDS)
def test_output_extents_are_ceil_half(s, kernel):
    n, cin, cout, H, W = cs.SHAPES[s]
    want = (n, cout, (H + 1) // 2, (W + 1) // 2)
    assert cs.out_extents(H, W) == want[2:]
    for with_res in (False, True):
        assert cs.exact_reference(s, kernel, with_res)["ref"].shape == want
    assert cs.random_reference(s, kernel, "bfloat16", True)["ref"].shape == want
    assert cs.exact_inputs(s, kernel)["res"].shape == want and cs.random_inputs(s, kernel)["res"].shape == want
    # torch's formula, floor((H + 2p - d(k - 1) - 1) / 2) + 1
    p = 1 if kernel == 3 else 0
    assert ((H + 2 * p - (kernel - 1) - 1) // 2 + 1, (W + 2 * p - (kernel - 1) - 1) // 2 + 1) == want[2:]


def _sampled(x, w, kernel):
    """The contract's sum written out: w[co][ci][ky][kx] * in[n][ci][2y + ky - 1][2x + kx - 1] (1x1: in[2y][2x]), a
    tap outside the image contributing nothing; float64 numpy."""
    n, cin, H, W = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    out = np.zeros((n, w.shape[0], Ho, Wo))
    off = 1 if kernel == 3 else 0
    for y in range(Ho):
        for xx in range(Wo):
            for ky in range(kernel):
                for kx in range(kernel):
                    iy, ix = 2 * y + ky - off, 2 * xx + kx - off
                    if 0 <= iy < H and 0 <= ix < W:
                        out[:, :, y, xx] += x[:, :, iy, ix] @ w[:, :, ky, kx].T
    return out


@pytest.mark.parametrize("s, kernel", [(0, 3), (0, 1), (2, 3), (3, 3), (3, 1), (4, 3), (4, 1), (6, 3)])
def test_reference_is_the_contracts_sum_written_out(s, kernel):
    c = cs.exact_inputs(s, kernel)
    a, _ = cs.conv64(torch.from_numpy(c["x"].astype(np.float64)), torch.from_numpy(c["m"] / 256.0), kernel)
    assert np.array_equal(a.numpy(), _sampled(c["x"].astype(np.float64), c["m"] / 256.0, kernel))


def _fold64(bn):
    scale = (bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)).detach()
    return scale.numpy(), (bn.bias.double() - bn.running_mean.double() * scale).detach().numpy()


@pytest.mark.parametrize("rows, cols", [(9, 11), (8, 12), (1, 1)])
def test_reference_is_the_strided_basic_block_of_the_reference_model(rows, cols):
    """The block in float64 and eval mode against three calls of the reference with unrounded operands."""
    block = Block(16, 32, dilation=(1, 1), downsample=True, stride=2, seed=60).double().eval()
    x = torch.randn(2, 16, rows, cols, generator=torch.Generator().manual_seed(61)).double()
    with torch.no_grad():
        want = block(x)
    y = cs.reference(x.numpy(), block.conv1.weight.detach().numpy(), *_fold64(block.bn1), 3, None)["ref"]
    res = cs.reference(x.numpy(), block.downsample[0].weight.detach().numpy(), *_fold64(block.downsample[1]), 1, None,
                       relu=False)["ref"]
    got = cb.reference(y, block.conv2.weight.detach().numpy(), *_fold64(block.bn2), 3, 1, None, residual=res)
    assert got["ref"].shape == tuple(want.shape) == (2, 32, (rows + 1) // 2, (cols + 1) // 2)
    assert np.allclose(got["ref"], want.numpy(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("dtype", sorted(cs.DTYPES))
@pytest.mark.parametrize("s, kernel", KERNEL_CASES, ids=KERNEL_IDS)
def test_exact_inputs_are_exact(s, kernel, dtype):
    """Both half dtypes hold the features and the residual as given and round the weights back to m / 256; every
    value of the float64 reference, before and after each step of the epilogue, is a multiple of 2^-9 below 2^15 and
    an fp32 value."""
    c = cs.exact_inputs(s, kernel)
    for name in ("x", "res"):
        assert torch.equal(cr.round_half(c[name], dtype), torch.from_numpy(c[name].astype(np.float64)))
    assert np.abs(c["res"]).max() <= 8 and c["x"].max() <= 3 and c["x"].min() >= 0
    assert torch.equal(cr.round_half(c["w"], dtype), torch.from_numpy(c["m"] / 256.0))
    assert not np.array_equal(c["w"].astype(np.float64), c["m"] / 256.0)      # (the pack call has to round)
    assert set(np.abs(c["scale"]).tolist()) <= {0.5, 1.0, 2.0}
    assert np.array_equal(c["shift"], np.round(c["shift"])) and np.abs(c["shift"]).max() <= 4
    for with_res in (False, True):
        for relu in (True, False):
            r = cs.exact_reference(s, kernel, with_res, relu)
            assert r["A"].max() < 2.0 ** 14
            for name in ("ref", "pre", "prerelu"):
                assert np.abs(r[name]).max() < 2.0 ** 15
                assert np.array_equal(r[name] * 512.0, np.round(r[name] * 512.0))
                assert np.array_equal(r[name].astype(np.float32).astype(np.float64), r[name])
    # the same reference from the generic path on the rounded operands
    g = cs.reference(c["x"], c["w"], c["scale"], c["shift"], kernel, dtype, residual=c["res"])
    assert np.array_equal(g["ref"], cs.exact_reference(s, kernel, True)["ref"])


def _contract_fp32(c, dtype, kernel, residual, relu=True, wrong=None):
    """The contract evaluated in fp32 on the CPU (torch's strided convolution in fp32, then the epilogue step by step
    in numpy fp32), or one of three wrong forms of it."""
    x32, w32 = cr.round_half(c["x"], dtype).float(), cr.round_half(c["w"], dtype).float()
    n, cin, H, W = x32.shape
    Ho, Wo = cs.out_extents(H, W)
    pad = 1 if kernel == 3 else 0
    if wrong == "no_minus_one":
        # in[2y + ky][2x + kx], the taps one pixel down and right of the contract's (the 1x1 form, which has no -1 to
        # forget, one pixel down and right as well: in[2y + 1][2x + 1]); zeros outside the image
        shifted = x32 if kernel == 3 else x32[:, :, 1:, 1:]
        a = F.conv2d(F.pad(shifted, (0, 3, 0, 3)), w32, stride=2)[:, :, :Ho, :Wo].numpy()
    else:
        a = F.conv2d(x32, w32, stride=2, padding=pad).numpy()
    v = (c["scale"].reshape(1, -1, 1, 1) * a + c["shift"].reshape(1, -1, 1, 1)).astype(np.float32)
    if residual is not None:
        res = cr.round_half(residual, dtype).float().numpy()
        if wrong == "input_pitch":         # residual[(.. * Ho + y) * W + x]: the input's row pitch on the output's buffer
            flat = res.reshape(-1)
            idx = (np.arange(n * res.shape[1] * Ho).reshape(-1, 1) * W + np.arange(Wo).reshape(1, -1)) % flat.size
            res = flat[idx].reshape(res.shape)
        v = (v + res).astype(np.float32)
    v = np.maximum(v, np.float32(0)) if relu else v
    if wrong == "floor_extent":            # rows_in // 2 x cols_in // 2 written, the rest of the output left zero
        v[:, :, H // 2:, :] = 0
        v[:, :, :, W // 2:] = 0
    return v


def _ratio(c, dtype, kernel, r, residual, **kw):
    return (np.abs(_contract_fp32(c, dtype, kernel, residual, **kw).astype(np.float64) - r["ref"]) / r["tol"]).max()


@pytest.mark.parametrize("kernel", cs.KERNELS)
def test_bound_catches_wrong_strides_and_passes_fp32(kernel):
    """At the first shape (2 x 16 -> 32 x 5 x 7, output 3 x 4): an fp32 evaluation of the contract stays far inside the
    bound; sampling without the -1, an output extent of rows_in // 2 with the rest zero, and a residual read with the
    input's row pitch are each far outside it."""
    s = 0
    c = cs.random_inputs(s, kernel)
    for dtype in sorted(cs.DTYPES):
        for with_res in (False, True):
            r = cs.random_reference(s, kernel, dtype, with_res)
            res = c["res"] if with_res else None
            assert _ratio(c, dtype, kernel, r, res) < 0.2
            for wrong in ("no_minus_one", "floor_extent") + (("input_pitch",) if with_res else ()):
                bad = _ratio(c, dtype, kernel, r, res, wrong=wrong)
                assert bad > 10, (wrong, bad)
        r0 = cs.random_reference(s, kernel, dtype, True, relu=False)
        assert _ratio(c, dtype, kernel, r0, c["res"], relu=False) < 0.2 and (r0["ref"] < 0).any()


@pytest.mark.parametrize("s, kernel", KERNEL_CASES, ids=KERNEL_IDS)
def test_fp32_evaluation_stays_inside_the_bound_at_every_shape(s, kernel):
    c = cs.random_inputs(s, kernel)
    for dtype in sorted(cs.DTYPES):
        for with_res in (False, True):
            r = cs.random_reference(s, kernel, dtype, with_res)
            assert _ratio(c, dtype, kernel, r, c["res"] if with_res else None) < 0.2


# ---- cnn.StridedResidualBlock: every refusal is made before anything is packed, so none needs a device ----

class _Bottleneck(Block):
    def __init__(self):
        super().__init__(32, 64, dilation=(1, 1), downsample=True, stride=2)
        self.conv3 = torch.nn.Conv2d(64, 64, 1, bias=False)


def _strided(**kw):
    return Block(32, 64, dilation=kw.pop("dilation", (1, 1)), downsample=kw.pop("downsample", True),
                 stride=kw.pop("stride", 2), **kw).eval()


def _downsample_stride(block, stride):
    block.downsample[0].stride = (stride, stride)
    return block


def _training_downsample():
    block = _strided()
    block.downsample[1].train()
    return block


def _strided_conv2():
    block = _strided()
    block.conv2.stride = (2, 2)
    return block


REFUSALS = [
    (lambda: Block(32, 32, dilation=(1, 1), stride=2).eval(), "conv1 has stride 2 and the block no downsample"),
    (lambda: _downsample_stride(_strided(), 1), r"downsample has stride \(1, 1\), conv1 \(2, 2\)"),
    (lambda: _downsample_stride(_strided(stride=1), 2), r"downsample has stride \(2, 2\), conv1 \(1, 1\)"),
    (lambda: _strided(dilation=(2, 2)), "stride 2 with dilation 2"),
    (lambda: _strided(stride=3), r"conv1 has stride \(3, 3\)"),
    (lambda: _strided_conv2(), r"conv2 has stride \(2, 2\)"),
    (lambda: _strided().train(), "eval"),
    (lambda: _training_downsample(), "eval"),
    (lambda: _Bottleneck().eval(), "Bottleneck"),
]


@pytest.mark.parametrize("make, message", REFUSALS)
def test_strided_residual_block_refusals_need_no_device(make, message, monkeypatch):
    def touched(*args, **kwargs):
        raise AssertionError("weights were packed before the refusal")
    monkeypatch.setattr(core, "conv_pack_weights", touched)
    with pytest.raises(core.CoreError, match=message):
        cnn.StridedResidualBlock(make())


def test_residual_block_still_refuses_strides():
    with pytest.raises(core.CoreError, match="stride"):
        cnn.ResidualBlock(_strided())
    with pytest.raises(core.CoreError, match="downsample has stride"):
        cnn.ResidualBlock(_downsample_stride(_strided(stride=1), 2))
    assert cnn.ResidualBlock.strides == (1,) and cnn.StridedResidualBlock.strides == (1, 2)
    # one body: the subclass adds the allowed strides and nothing else
    assert set(vars(cnn.StridedResidualBlock)) <= {"strides", "__doc__", "__module__"}
    layer2 = torch.nn.Sequential(torch.nn.Conv2d(16, 32, 3, stride=2, padding=1, bias=False), _bn(32, 1),
                                 torch.nn.ReLU()).eval()
    with pytest.raises(core.CoreError, match="stride"):
        cnn.ConvBnRelu(layer2[0], layer2[1])


SIGNATURES = [
    (core.conv_bn_stride_ptr, "(stream=0, **fields)"),
    (core.conv_bn_stride, "(features, packed, scale, shift, kernel, stride, dilation=1, residual=None, relu=True, "
                          "out_dtype=None, canary=0)"),
    (cnn.ConvBn.__init__, "(self, weight, fold, kernel, dilation, relu, dtype, dev, stride=1)"),
    (cnn.StridedResidualBlock.__init__, "(self, block, dtype=torch.bfloat16, device=0)"),
    (cnn.DrnDownsampling.__init__, "(self, layer2, layer3, layer4, layer5, layer6, layer7, layer8, seg, n_classes, "
                                   "rows_power2_segmentation, clamp=None, dtype=torch.bfloat16, device=0)"),
    (cnn.DrnDownsampling.forward, "(self, features, want_cnn_out=False)"),
]


@pytest.mark.parametrize("fn, signature", SIGNATURES, ids=[fn.__qualname__ for fn, _ in SIGNATURES])
def test_public_signatures_are_pinned(fn, signature):
    assert str(inspect.signature(fn)) == signature

