"""The backbone tail (f17) without a GPU: the symbols and bindings, the struct layout, the ranges of
is_conv3x3_packed_bytes, the refusals of is_conv3x3_bn_relu and is_conv3x3_pack_weights (all made before the device is
touched), cnn.fold_batchnorm, and the reference of tests/conv3x3_reference.py pinned against torch's own modules and
against the claim that its exact inputs are exact."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import conv3x3_reference as cr
from instance_stixels_amd import cnn, core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("is_conv3x3_packed_bytes", "is_conv3x3_pack_weights", "is_conv3x3_bn_relu")


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "instance_stixels_core.h")).read()
    for name in NAMES:
        assert name + "(" in header, name
        assert name in core.EXPORTS and hasattr(core.lib(), name), name
    for fn in ("conv3x3_packed_bytes", "conv3x3_pack_weights", "conv3x3_bn_relu", "conv3x3_bn_relu_ptr"):
        assert callable(getattr(core, fn)), fn
    for cite in ("drn.py:181-185", "drn.py:223-233", "inference.py:278"):
        assert cite in header, cite
    # the contract stands in the header and in the kernel's top comment
    kernel = open(os.path.join(ROOT, "instance_stixels_amd", "csrc", "is_k_conv3x3.hip")).read()
    for text in (header, kernel):
        assert "v_mfma_f32_32x32x16" in text and "not specified" in text and "fmaf(scale[co], a, shift[co])" in text
    assert "is_k_conv3x3.hip" in open(os.path.join(ROOT, "instance_stixels_amd", "csrc", "Makefile")).read()


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "instance_stixels_core.h"
#define F(f) printf(#f " %zu %zu\n", offsetof(is_conv3x3_args, f), sizeof(((is_conv3x3_args*)0)->f));
int main() {
    printf(". %zu 0\n", sizeof(is_conv3x3_args));
    FIELDS
    return 0;
}
"""


def test_args_layout_matches_the_header(tmp_path):
    src = PROBE.replace("FIELDS", "".join(f"F({n})" for n, _ in core.Conv3x3Args._fields_))
    (tmp_path / "probe.cpp").write_text(src)
    exe = str(tmp_path / "probe")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "probe.cpp"), "-o", exe],
                   check=True)
    got = {f: (int(off), int(size)) for f, off, size in
           (l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())}
    assert got["."][0] == ctypes.sizeof(core.Conv3x3Args) == 104
    declared = re.search(r"typedef struct is_conv3x3_args \{(.*?)\} is_conv3x3_args;",
                         open(os.path.join(ROOT, "include", "instance_stixels_core.h")).read(), re.S).group(1)
    names = re.findall(r"(\w+)(?:\[4\])?\s*[,;]", declared)
    assert names == [n for n, _ in core.Conv3x3Args._fields_]
    for name, _ in core.Conv3x3Args._fields_:
        field = getattr(core.Conv3x3Args, name)
        assert got[name] == (field.offset, field.size), name


def test_packed_bytes_honours_the_ranges():
    pb = core.conv3x3_packed_bytes
    for dt in (core.HEAD_F16, core.HEAD_BF16):
        assert pb(32, 16, dt) == 32 * 16 * 9 * 2
        assert pb(512, 512, dt) == 512 * 512 * 9 * 2
        assert pb(2048, 2048, dt) == 2048 * 2048 * 9 * 2
        assert pb(64, 48, dt) == 64 * 48 * 9 * 2
        for cout, cin in ((0, 16), (16, 16), (48, 16), (2080, 16), (32, 0), (32, 8), (32, 24), (32, 2064), (-32, 16),
                          (32, -16)):
            assert pb(cout, cin, dt) == 0, (cout, cin)
    for dt in (core.HEAD_F32, 3, -1):
        assert pb(32, 16, dt) == 0


# A call that would be accepted (the pointers are never dereferenced on the host: every case below is refused before
# the device is touched, so this file needs no GPU).  Features 2*1*16*5*7 = 1120 B at 0x10000, output at 0x20000.
GOOD = dict(d_features=0x10000, dtype=core.HEAD_BF16, n_images=1, channels_in=16, channels_out=32, rows8=5, cols8=7,
            dilation=2, d_packed=0x30000, d_scale=0x40000, d_shift=0x50000, relu=1, d_out=0x20000,
            out_dtype=core.HEAD_BF16)


@pytest.mark.parametrize("change, message", [
    (dict(d_features=None), "null"),
    (dict(d_packed=None), "null"),
    (dict(d_scale=None), "null"),
    (dict(d_shift=None), "null"),
    (dict(d_out=None), "null"),
    (dict(dtype=core.HEAD_F32, out_dtype=core.HEAD_F32), "dtype"),
    (dict(dtype=3), "dtype"),
    (dict(dtype=-1), "dtype"),
    (dict(out_dtype=core.HEAD_F16), "out_dtype"),                            # a half, but not the input's
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
    (dict(d_features=0x10001), "aligned"),
    (dict(d_out=0x20002, out_dtype=core.HEAD_F32), "aligned"),
    (dict(d_out=0x10000), "overlap"),                                        # in place
    (dict(d_out=0x10000 + 1118), "overlap"),                                 # the features' last element
    (dict(d_out=0x10000 - 2240 + 2), "overlap"),                             # the output's last element
    (dict(reserved=(0, 0, 1, 0)), "reserved"),
])
def test_refusals_need_no_device(change, message):
    rc = core.conv3x3_bn_relu_ptr(**dict(GOOD, **change))
    assert rc == -1                                                          # IS_EINVAL
    assert re.search(message, core.lib().is_last_error().decode()), core.lib().is_last_error()


def test_null_args_and_pack_refusals():
    L = core.lib()
    assert L.is_conv3x3_bn_relu(None, None) == -1
    assert b"null args" in L.is_last_error()
    for args, message in (((None, 32, 16, core.HEAD_F16, 0x1000), b"null"),
                          ((0x1000, 32, 16, core.HEAD_F16, None), b"null"),
                          ((0x1000, 32, 16, core.HEAD_F32, 0x2000), b"dtype"),
                          ((0x1000, 48, 16, core.HEAD_F16, 0x2000), b"channels_out"),
                          ((0x1000, 32, 8, core.HEAD_F16, 0x2000), b"channels_in"),
                          ((0x1002, 32, 16, core.HEAD_F16, 0x2000), b"d_weight"),
                          ((0x1000, 32, 16, core.HEAD_F16, 0x2004), b"d_packed")):
        assert L.is_conv3x3_pack_weights(*args, None) == -1, args
        assert message in L.is_last_error(), (args, L.is_last_error())


# ---- fold_batchnorm ----

def _bn(channels, seed, affine=True):
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm2d(channels, affine=affine)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(channels, generator=g))
        bn.running_var.copy_(torch.rand(channels, generator=g) * 2 + 0.01)
        if affine:
            bn.weight.copy_(torch.randn(channels, generator=g))
            bn.bias.copy_(torch.randn(channels, generator=g) * 0.1)
    return bn.eval()


def test_fold_batchnorm_is_the_eval_mode_module():
    bn = _bn(32, seed=1)
    scale, shift = cnn.fold_batchnorm(bn)
    assert scale.dtype == shift.dtype == torch.float32 and scale.shape == shift.shape == (32,)
    # the formula in numpy float64, each value rounded once
    w, b = bn.weight.detach().numpy().astype(np.float64), bn.bias.detach().numpy().astype(np.float64)
    m, v = bn.running_mean.numpy().astype(np.float64), bn.running_var.numpy().astype(np.float64)
    s64 = w / np.sqrt(v + bn.eps)
    assert np.array_equal(scale.numpy(), s64.astype(np.float32))
    assert np.array_equal(shift.numpy(), (b - m * s64).astype(np.float32))
    # and the module itself in float64: the fold is within its two roundings of it
    x = torch.randn(2, 32, 3, 5, generator=torch.Generator().manual_seed(2)).double()
    with torch.no_grad():
        y = _bn(32, seed=1).double()(x)
    folded = scale.double().view(1, -1, 1, 1) * x + shift.double().view(1, -1, 1, 1)
    bound = 2.0 ** -24 * (scale.double().abs().view(1, -1, 1, 1) * x.abs() + shift.double().abs().view(1, -1, 1, 1)) + 1e-12
    assert ((folded - y).abs() <= bound).all()
    s1, h1 = cnn.fold_batchnorm(_bn(16, seed=3, affine=False))
    ref = _bn(16, seed=3, affine=False)
    assert np.array_equal(s1.numpy(), (1.0 / np.sqrt(ref.running_var.numpy().astype(np.float64) + ref.eps)).astype(np.float32))


def test_fold_batchnorm_raises_in_training_mode():
    bn = _bn(32, seed=1).train()
    with pytest.raises(core.CoreError, match="eval"):
        cnn.fold_batchnorm(bn)
    with pytest.raises(core.CoreError, match="BatchNorm"):
        cnn.fold_batchnorm(torch.nn.ReLU())


# ---- the reference against torch's own modules, and its exact inputs ----

@pytest.mark.parametrize("s", [0, 1, 2, 3], ids=cr.SHAPE_IDS[:4])
def test_reference_is_the_sequential_of_the_reference_model(s):
    """_make_conv_layers' Sequential(Conv2d(bias=False, padding=dilation, dilation), BatchNorm2d, ReLU) in float64
    and eval mode, on the exact inputs with a real BatchNorm: the reference module with the float64 fold agrees to
    float64 rounding."""
    n, cin, cout, H, W, d = cr.SHAPES[s]
    c = cr.exact_inputs(s)
    conv = torch.nn.Conv2d(cin, cout, 3, padding=d, dilation=d, bias=False)
    bn = _bn(cout, seed=10 + s)
    seq = torch.nn.Sequential(conv, bn, torch.nn.ReLU()).double().eval()
    w64 = torch.from_numpy(c["m"] / 256.0)
    with torch.no_grad():
        conv.weight.copy_(w64)
        want = seq(torch.from_numpy(c["x"].astype(np.float64)))
    scale64 = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).detach().numpy()
    shift64 = (bn.bias - bn.running_mean * torch.from_numpy(scale64)).detach().numpy()
    a, A = cr.conv64(torch.from_numpy(c["x"].astype(np.float64)), w64, d)
    got = cr.epilogue64(a, scale64, shift64, relu=True)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-9)
    assert (want > 0).any() and (want == 0).any()                # (ReLU does something)
    # with scale 1, shift 0 the reference is the convolution itself, bit for bit
    plain = torch.nn.functional.conv2d(torch.from_numpy(c["x"].astype(np.float64)), w64, padding=d, dilation=d)
    assert np.array_equal(cr.exact_reference(s, relu=False)["ref"], plain.numpy())


@pytest.mark.parametrize("dtype", sorted(cr.DTYPES))
@pytest.mark.parametrize("s", range(len(cr.SHAPES)), ids=cr.SHAPE_IDS)
def test_exact_inputs_are_exact(s, dtype):
    """Both half dtypes hold the features as given and round the weights back to m / 256; every product is a multiple
    of 2^-8 and sum |w x| stays below 2^14, so every partial sum in any order has at most 22 significant bits: exact
    in fp32, and the fp32 result is the float64 reference."""
    c, r = cr.exact_inputs(s), cr.exact_reference(s)
    assert torch.equal(cr.round_half(c["x"], dtype), torch.from_numpy(c["x"].astype(np.float64)))
    assert torch.equal(cr.round_half(c["w"], dtype), torch.from_numpy(c["m"] / 256.0))
    assert not np.array_equal(c["w"].astype(np.float64), c["m"] / 256.0)      # (the pack call has to round)
    assert r["A"].max() < 2.0 ** 14
    for name in ("ref", "A"):
        assert np.array_equal(r[name] * 256.0, np.round(r[name] * 256.0))
        assert np.array_equal(r[name].astype(np.float32).astype(np.float64), r[name])
    # the same reference from the generic path on the rounded operands
    if s < 4:
        g = cr.reference(c["x"], c["w"], c["scale"], c["shift"], cr.SHAPES[s][5], dtype)
        assert np.array_equal(g["ref"], r["ref"])


def test_bound_catches_a_dropped_term_and_passes_fp32():
    """At (16, 32, 5x7): an fp32 convolution of the random inputs stays far inside the bound, a single dropped term
    is far outside it."""
    s = 0
    n, cin, cout, H, W, d = cr.SHAPES[s]
    c = cr.random_inputs(s)
    for dtype in sorted(cr.DTYPES):
        r = cr.random_reference(s, dtype)
        x32, w32 = cr.round_half(c["x"], dtype).float(), cr.round_half(c["w"], dtype).float()
        a32 = torch.nn.functional.conv2d(x32, w32, padding=d, dilation=d)
        v32 = torch.clamp_min(torch.tensor(c["scale"]).view(1, -1, 1, 1) * a32 +
                              torch.tensor(c["shift"]).view(1, -1, 1, 1), 0.0)
        ratio = np.abs(v32.double().numpy() - r["ref"]) / r["tol"]
        assert ratio.max() < 0.1, ratio.max()
        # drop the centre tap of channel 0 at an interior pixel
        term = abs(float(w32[0, 0, 1, 1]) * float(x32[0, 0, 2, 3]) * float(c["scale"][0]))
        assert term > 10 * r["tol"][0, 0, 2, 3]
