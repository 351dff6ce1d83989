"""The segmentation head (f13) without a GPU: the symbols and bindings, the refusals of is_segmentation_head (all made
before the device is touched), the host class's size checks, and the reference of tests/head_reference.py pinned
against torch's modules on the CPU."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import head_reference as hr
from instance_stixels_amd import core, host, make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "instance_stixels_core.h")).read()
    assert "is_segmentation_head(" in header
    assert "is_segmentation_head" in core.EXPORTS and hasattr(core.lib(), "is_segmentation_head")
    for name in ("ish_set_segmentation_head", "ish_segmentation_head_batch"):
        assert name in host.EXPORTS and hasattr(host.lib(), name), name
    for name in ("SetSegmentationHead", "SegmentationHeadBatch"):
        assert callable(getattr(host.Stixels, name)), name
    assert callable(core.segmentation_head) and callable(core.segmentation_head_ptr)
    for name, value in (("F32", core.HEAD_F32), ("F16", core.HEAD_F16), ("BF16", core.HEAD_BF16),
                        ("MAX_CHANNELS", core.HEAD_MAX_CHANNELS)):
        assert int(re.search(rf"#define IS_HEAD_{name} (\d+)", header).group(1)) == value
    for cite in ("DRNDownsampled.py:97-102", ":128-137", "wrappers.py:35-61", "inference.py:374"):
        assert cite in header, cite


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "instance_stixels_core.h"
#define F(f) printf(#f " %zu %zu\n", offsetof(is_segmentation_head_args, f), sizeof(((is_segmentation_head_args*)0)->f));
int main() {
    printf(". %zu 0\n", sizeof(is_segmentation_head_args));
    FIELDS
    return 0;
}
"""


def test_args_layout_matches_the_header(tmp_path):
    src = PROBE.replace("FIELDS", "".join(f"F({n})" for n, _ in core.SegmentationHeadArgs._fields_))
    (tmp_path / "probe.cpp").write_text(src)
    exe = str(tmp_path / "probe")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "probe.cpp"), "-o", exe],
                   check=True)
    got = {f: (int(off), int(size)) for f, off, size in
           (l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())}
    assert got["."][0] == ctypes.sizeof(core.SegmentationHeadArgs)
    for name, _ in core.SegmentationHeadArgs._fields_:
        field = getattr(core.SegmentationHeadArgs, name)
        assert got[name] == (field.offset, field.size), name


# A call that would be accepted (the pointers are never dereferenced on the host: every case below is refused before
# the device is touched, so this file needs no GPU).
GOOD = dict(d_features=0x1000, dtype=core.HEAD_F32, n_images=1, K=16, rows8=7, cols8=9, d_weight=0x2000, d_bias=0x3000,
            n_classes=19, n_regression=2, rows_power2_segmentation=8, d_cnn_out=0x4000, d_segmentation=0x5000)


@pytest.mark.parametrize("change, message", [
    (dict(d_cnn_out=None, d_segmentation=None), "both null"),
    (dict(n_classes=19, n_regression=14), "IS_HEAD_MAX_CHANNELS"),          # channels_out = 33
    (dict(n_classes=0, n_regression=21), "n_classes"),
    (dict(K=12), "multiple of 8"),
    (dict(K=0), "multiple of 8"),
    (dict(rows8=8, rows_power2_segmentation=8), "rows8 \\+ 1"),             # P2S = rows8
    (dict(rows_power2_segmentation=24), "power of two"),
    (dict(reserved=(0, 0, 1, 0)), "reserved"),
    (dict(dtype=3), "dtype"),
    (dict(dtype=-1), "dtype"),
    (dict(d_features=None), "null"),
    (dict(n_images=0), "n_images"),
    (dict(cols8=0), "cols8"),
    (dict(clamp_channel=0, clamp_lo=0.0, clamp_hi=1.0), "clamp_channel"),   # a class channel
    (dict(clamp_channel=21), "clamp_channel"),
    (dict(clamp_channel=19, clamp_lo=2.0, clamp_hi=1.0), "clamp_lo"),
    (dict(d_features=0x1002), "aligned"),
])
def test_refusals_need_no_device(change, message):
    rc = core.segmentation_head_ptr(**dict(GOOD, **change))
    assert rc == -1                                                          # IS_EINVAL
    assert re.search(message, core.lib().is_last_error().decode()), core.lib().is_last_error()


def test_null_args_are_refused():
    assert core.lib().is_segmentation_head(None, None) == -1
    assert b"null args" in core.lib().is_last_error()


def test_set_segmentation_head_checks_sizes():
    cfg = make_config("drn_d_22_unary", 128, 256, 32)
    st = host.Stixels()
    st.SetConfig(cfg)                                                         # 19 classes + 2 instance channels
    w, b = np.zeros((21, 16), np.float32), np.zeros(21, np.float32)
    st.SetSegmentationHead(w, b, 16)
    with pytest.raises(ValueError, match="bias.size"):
        st.SetSegmentationHead(np.zeros((20, 16), np.float32), np.zeros(20, np.float32), 16)
    with pytest.raises(ValueError, match="weight.size"):
        st.SetSegmentationHead(np.zeros((21, 24), np.float32), b, 16)
    with pytest.raises(ValueError, match="multiple of 8"):
        st.SetSegmentationHead(np.zeros((21, 12), np.float32), b, 12)
    with pytest.raises(ValueError, match="lo must be <= hi"):
        st.SetSegmentationHeadClamp(19, 2.0, 1.0)
    with pytest.raises(ValueError, match="not initialised"):
        st.SegmentationHeadBatch(1, 0x1000, core.HEAD_F32, 0x2000)


# ---- the reference against torch's own modules ----

def _torch_head(x, w, b, n_classes):
    """DRNDSDoubleSeg's head built by hand (DRNDownsampled.py:80-102) in float64: Conv2d 1x1 with the given weights,
    LogSoftmax(dim=1) on the class channels, the negation (the sign of inference.py:374), the concatenation."""
    import torch
    C, K = w.shape
    seg = torch.nn.Conv2d(K, C, kernel_size=1, bias=True).double()
    with torch.no_grad():
        seg.weight.copy_(torch.from_numpy(w.astype(np.float64)).reshape(C, K, 1, 1))
        seg.bias.copy_(torch.from_numpy(b.astype(np.float64)))
        y = seg(torch.from_numpy(x.astype(np.float64)))
        out = torch.cat((-torch.nn.LogSoftmax(dim=1)(y[:, :n_classes]), y[:, n_classes:]), dim=1)
    return y.numpy(), out.numpy()


def _reference_init(K, channels, seed):
    """`seg` as the reference initialises it (DRNDownsampled.py:82-85): N(0, sqrt(2 / n)), n = 1 * 1 * out_channels;
    bias zero."""
    import torch
    torch.manual_seed(seed)
    m = torch.nn.Conv2d(K, channels, kernel_size=1, bias=True)
    n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
    m.weight.data.normal_(0, math.sqrt(2.0 / n))
    m.bias.data.zero_()
    return m.weight.detach().numpy().reshape(channels, K).copy(), m.bias.detach().numpy().copy()


@pytest.mark.parametrize("K", [8, 24, 512])
def test_reference_is_exact_on_exact_inputs(K):
    """Features multiples of 1/8 in [0, 4), weights and bias multiples of 1/64 in [-1, 1], K <= 512: every product and
    every partial sum is a multiple of 2^-9 below 2^12, exact in fp32 in any order.  Then the reference's logits ARE
    the float64 logits, its regression channels equal torch's bitwise after one rounding, and its class channels stay
    within the class bound of torch's -log_softmax."""
    rng = np.random.default_rng(K)
    n, Hs, Ws, C, ncls = 2, 5, 7, 21, 19
    x = (rng.integers(0, 32, (n, K, Hs, Ws)) / 8.0).astype(np.float32)
    w = (rng.integers(-64, 65, (C, K)) / 64.0).astype(np.float32)
    b = (rng.integers(-64, 65, C) / 64.0).astype(np.float32)
    z = hr.logits(x, w, b)
    y64, out64 = _torch_head(x, w, b, ncls)
    assert np.array_equal(z.astype(np.float64), y64)
    ref = hr.cnn_out(z, ncls)
    assert np.array_equal(ref[:, ncls:].view(np.uint32), out64[:, ncls:].astype(np.float32).view(np.uint32))
    err = np.abs(ref[:, :ncls].astype(np.float64) - out64[:, :ncls])
    assert (err <= hr.class_tolerance(z, ncls)).all(), err.max()
    # the int tensor is FlipAndPad's (wrappers.py:35-61) of that output: permute(0, 3, 1, 2), flip, pad, * 8, int
    import torch
    t = torch.from_numpy(ref).permute(0, 3, 1, 2).flip(3)
    t = (torch.nn.functional.pad(t, (0, 8 - Hs)) * 8).int().numpy()
    assert np.array_equal(hr.segmentation(ref, 8), t)


def test_reference_logits_stay_within_the_chain_bound():
    """Random inputs with the reference's init: |fmaf chain - float64 dot product| <= K 2^-24 sum_k |w x| (K roundings,
    each at most half an ulp of a partial sum that sum_k |w x| + |bias| bounds; the bias term is inside the slack of
    the factor two between 2^-24 and half an ulp's 2^-25 ... 2^-24)."""
    K, C = 512, 21
    w, _ = _reference_init(K, C, seed=1)
    rng = np.random.default_rng(2)
    x = np.abs(rng.standard_normal((1, K, 6, 11))).astype(np.float32)
    b = (rng.standard_normal(C) * 0.1).astype(np.float32)
    z = hr.logits(x, w, b)
    w64, x64 = w.astype(np.float64), x.astype(np.float64)
    exact = np.einsum("ck,nkhw->nchw", w64, x64) + b.astype(np.float64)[None, :, None, None]
    mag = np.einsum("ck,nkhw->nchw", np.abs(w64), x64)
    assert (np.abs(z.astype(np.float64) - exact) <= K * 2.0 ** -24 * mag).all()
    assert (z.astype(np.float64) != exact).any()       # (the bound is not vacuous: fp32 does round here)


def test_reference_clamp_and_dominant_class():
    z = np.zeros((1, 22, 2, 3), np.float32)
    z[0, 19] = np.array([[-3.0, 0.5, 200.0], [128.0, 129.0, -0.0]], np.float32)
    z[0, 3] += 40.0
    out = hr.cnn_out(z, 19, clamp=(19, 0.0, 128.0))
    assert out[0, 19].tolist() == [[0.0, 0.5, 128.0], [128.0, 128.0, 0.0]]
    # the true value is log1p(18 e^-40), about 7.6e-17; the contract's binary64 expression gives 0 there (1 + 7.6e-17
    # rounds to 1), which the floor of the class bound covers
    assert (out[0, 3] >= 0).all() and (out[0, 3] <= hr.class_tolerance(z, 19)[0, 3]).all()
    assert np.allclose(out[0, 0], 40.0)
