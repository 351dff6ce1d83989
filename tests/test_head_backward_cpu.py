"""The head's backward pass and the semantic NLL loss (f14) without a GPU: the symbols and bindings, the struct
layouts, the refusals of both entries (all made before the device is touched), and the reference of
tests/head_backward_reference.py pinned against torch.autograd in float64 on the CPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import head_backward_reference as hbr
import head_reference as hr
from instance_stixels_amd import core, training

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("is_segmentation_head_backward_scratch_bytes", "is_segmentation_head_backward",
         "is_semantic_nll_scratch_bytes", "is_semantic_nll")


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "instance_stixels_core.h")).read()
    for name in NAMES:
        assert name + "(" in header, name
        assert name in core.EXPORTS and hasattr(core.lib(), name), name
    for name in ("segmentation_head_backward", "segmentation_head_backward_ptr", "semantic_nll", "semantic_nll_ptr",
                 "segmentation_head_backward_scratch_bytes", "semantic_nll_scratch_bytes"):
        assert callable(getattr(core, name)), name
    chunk = int(re.search(r"#define IS_HEAD_BACKWARD_CHUNK (\d+)", header).group(1))
    assert chunk == core.HEAD_BACKWARD_CHUNK and chunk % 64 == 0
    assert header.index("---- f13:") < header.index("---- f14:")
    for cite in ("train.py:698-732", "train.py:281-282", "DRNDownsampled.py:139-143", "DRNDownsampled.py:133-134"):
        assert cite in header, cite
    assert issubclass(training.SegmentationHead, __import__("torch").nn.Module)
    assert callable(training.SemanticNLLLoss)


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "instance_stixels_core.h"
#define F(f) printf(#f " %zu %zu\n", offsetof(STRUCT, f), sizeof(((STRUCT*)0)->f));
int main() {
    printf(". %zu 0\n", sizeof(STRUCT));
    FIELDS
    return 0;
}
"""


@pytest.mark.parametrize("struct, cls", [("is_segmentation_head_backward_args", core.SegmentationHeadBackwardArgs),
                                         ("is_semantic_nll_args", core.SemanticNllArgs)])
def test_args_layout_matches_the_header(tmp_path, struct, cls):
    src = PROBE.replace("FIELDS", "".join(f"F({n})" for n, _ in cls._fields_)).replace("STRUCT", struct)
    (tmp_path / "probe.cpp").write_text(src)
    exe = str(tmp_path / "probe")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "probe.cpp"), "-o", exe],
                   check=True)
    got = {f: (int(off), int(size)) for f, off, size in
           (l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())}
    assert got["."][0] == ctypes.sizeof(cls)
    for name, _ in cls._fields_:
        field = getattr(cls, name)
        assert got[name] == (field.offset, field.size), name


# Calls that would be accepted (the pointers are never dereferenced on the host: every case below is refused before the
# device is touched).  7 * 9 * 21 = 1323 elements per frame.
BIG = 1 << 40
GOOD = dict(d_features=0x1000, dtype=core.HEAD_F32, n_images=2, K=16, rows8=7, cols8=9, d_weight=0x2000, n_classes=19,
            n_regression=2, d_cnn_out=0x3000, d_grad_out=0x4000, grad_image_stride=1323, d_grad_features=0x5000,
            d_grad_weight=0x6000, d_grad_bias=0x7000, d_grad_logits=0x8000, d_scratch=0x10000, scratch_bytes=BIG)


@pytest.mark.parametrize("change, message", [
    (dict(d_features=None), "null"),
    (dict(d_weight=None), "null"),
    (dict(d_cnn_out=None), "null"),
    (dict(d_grad_out=None), "null"),
    (dict(d_grad_features=None, d_grad_weight=None, d_grad_bias=None, d_grad_logits=None), "all null"),
    (dict(dtype=3), "dtype"),
    (dict(dtype=-1), "dtype"),
    (dict(n_images=0), "n_images"),
    (dict(n_images=65536), "n_images"),
    (dict(rows8=0), "rows8"),
    (dict(cols8=0), "cols8"),
    (dict(rows8=1 << 15, cols8=(1 << 14) + 1, grad_image_stride=BIG), "2\\^28"),
    (dict(K=12), "multiple of 8"),
    (dict(K=0), "multiple of 8"),
    (dict(n_classes=0, n_regression=21), "n_classes"),
    (dict(n_regression=-1), "n_regression"),
    (dict(n_classes=19, n_regression=14), "IS_HEAD_MAX_CHANNELS"),
    (dict(grad_image_stride=1322), "grad_image_stride"),
    (dict(reserved=(0, 0, 0, 1)), "reserved"),
    (dict(d_features=0x1002), "aligned"),
    (dict(d_grad_features=0x5002), "aligned"),
    (dict(dtype=core.HEAD_BF16, d_features=0x1001), "aligned"),
    (dict(d_grad_weight=0x6002), "aligned"),
    (dict(d_grad_out=0x4001), "aligned"),
    (dict(d_scratch=None), "null d_scratch"),
    (dict(d_scratch=0x10008), "16-byte"),
    (dict(scratch_bytes=core.segmentation_head_backward_scratch_bytes(2, 16, 7, 9, 21) - 1), "scratch_bytes"),
])
def test_backward_refusals_need_no_device(change, message):
    rc = core.segmentation_head_backward_ptr(**dict(GOOD, **change))
    assert rc == -1                                                          # IS_EINVAL
    assert re.search(message, core.lib().is_last_error().decode()), core.lib().is_last_error()


NLL_GOOD = dict(d_cnn_out=0x1000, cnn_image_stride=1323, d_target=0x2000, target_dtype=core.DTYPE_UINT8,
                ignore_index=255, n_images=2, rows8=7, cols8=9, n_classes=19, d_loss=0x3000, d_valid_count=0x3100,
                d_bad_count=0x3200, d_grad=0x4000, grad_image_stride=1197, d_scratch=0x10000, scratch_bytes=BIG)


@pytest.mark.parametrize("change, message", [
    (dict(d_cnn_out=None), "null"),
    (dict(d_target=None), "null"),
    (dict(d_loss=None), "null"),
    (dict(d_valid_count=None), "null"),
    (dict(d_bad_count=None), "null"),
    (dict(target_dtype=core.DTYPE_UINT16), "target_dtype"),
    (dict(target_dtype=7), "target_dtype"),
    (dict(n_images=0), "n_images"),
    (dict(rows8=0), "rows8"),
    (dict(rows8=1 << 15, cols8=(1 << 14) + 1, cnn_image_stride=BIG, grad_image_stride=BIG), "2\\^28"),
    (dict(n_images=16, rows8=1 << 14, cols8=1 << 14, cnn_image_stride=BIG, grad_image_stride=BIG), "31 bits"),
    (dict(n_classes=0), "n_classes"),
    (dict(n_classes=33, cnn_image_stride=BIG, grad_image_stride=BIG), "n_classes"),
    (dict(cnn_image_stride=1196), "cnn_image_stride"),
    (dict(grad_image_stride=1196), "grad_image_stride"),
    (dict(reserved=(1, 0, 0, 0)), "reserved"),
    (dict(d_cnn_out=0x1002), "aligned"),
    (dict(d_grad=0x4002), "aligned"),
    (dict(target_dtype=core.DTYPE_INT32, d_target=0x2002), "aligned"),
    (dict(d_scratch=None), "null d_scratch"),
    (dict(d_scratch=0x10004), "16-byte"),
    (dict(scratch_bytes=core.semantic_nll_scratch_bytes(2, 7, 9) - 1), "scratch_bytes"),
])
def test_nll_refusals_need_no_device(change, message):
    rc = core.semantic_nll_ptr(**dict(NLL_GOOD, **change))
    assert rc == -1
    assert re.search(message, core.lib().is_last_error().decode()), core.lib().is_last_error()


def test_null_args_are_refused():
    assert core.lib().is_segmentation_head_backward(None, None) == -1
    assert b"null args" in core.lib().is_last_error()
    assert core.lib().is_semantic_nll(None, None) == -1
    assert b"null args" in core.lib().is_last_error()


def test_scratch_bytes():
    T = core.HEAD_BACKWARD_CHUNK
    sb = core.segmentation_head_backward_scratch_bytes
    for bad in ((0, 16, 7, 9, 21), (65536, 16, 7, 9, 21), (1, 12, 7, 9, 21), (1, 0, 7, 9, 21), (1, 16, 0, 9, 21),
                (1, 16, 7, 0, 21), (1, 16, 7, 9, 0), (1, 16, 7, 9, 33), (1, 16, 1 << 15, (1 << 14) + 1, 21)):
        assert sb(*bad) == 0, bad
    # dz of the batch (padded to 16 bytes) and the chunk partials [n][chunks][CH][K + 1]
    assert sb(2, 16, 7, 9, 21) == (2 * 21 * 63 * 4 + 15) // 16 * 16 + 2 * 1 * 21 * 17 * 4
    assert sb(1, 512, 1, 2 * T + 37, 21) == (21 * (2 * T + 37) * 4 + 15) // 16 * 16 + 3 * 21 * 513 * 4
    nb = core.semantic_nll_scratch_bytes
    for bad in ((0, 7, 9), (65536, 7, 9), (1, 0, 9), (1, 7, 0), (1, 1 << 15, (1 << 14) + 1), (16, 1 << 14, 1 << 14)):
        assert nb(*bad) == 0, bad
    assert nb(2, 7, 9) > 0 and nb(2, 7, 9) % 16 == 0


# ---- the reference against torch.autograd in float64 ----

def _reference_step(x, w, b, n_classes, target, reg_grad, chunk):
    """The same step through the reference: (loss, dX, dW, db, y, gy, dz)."""
    z = hr.logits(x, w, b)
    y = hr.cnn_out(z, n_classes)
    loss, V, bad, gcls = hbr.nll64(y, target, n_classes)
    gy = np.concatenate((gcls, reg_grad.astype(np.float32)), axis=1)
    dz = hbr.dz(y, gy, n_classes)
    dW, db = hbr.grad_weight_bias(x, dz, chunk)
    return loss, hbr.grad_features(w, dz), dW, db, y, gy, dz


@pytest.mark.parametrize("K, chunk", [(8, 64), (24, 64), (512, 2048)])
def test_reference_chains_are_exact_on_exact_inputs(K, chunk):
    """Features multiples of 1/8 in [0, 4), weights multiples of 1/64 in [-1, 1], dz multiples of 1/16 in [-2, 2]:
    every product is a multiple of 2^-10 (dX) or 2^-7 (dW) and every partial sum stays below 2^13, exact in fp32 in
    any order.  Then the chains ARE torch.autograd's float64 gradients of the 1x1 convolution, split or not."""
    import torch
    rng = np.random.default_rng(K)
    n, Hs, Ws, C = 2, 5, 37, 21                                 # P = 185: three chunks of 64, the last one short
    x = (rng.integers(0, 32, (n, K, Hs, Ws)) / 8.0).astype(np.float32)
    w = (rng.integers(-64, 65, (C, K)) / 64.0).astype(np.float32)
    dz = (rng.integers(-32, 33, (n, C, Hs, Ws)) / 16.0).astype(np.float32)
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    wt = torch.from_numpy(w.astype(np.float64)).reshape(C, K, 1, 1).requires_grad_(True)
    bt = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(xt, wt, bt).backward(torch.from_numpy(dz.astype(np.float64)))
    dW, db = hbr.grad_weight_bias(x, dz, chunk)
    assert np.array_equal(hbr.grad_features(w, dz).astype(np.float64), xt.grad.numpy())
    assert np.array_equal(dW.astype(np.float64), wt.grad.numpy().reshape(C, K))
    assert np.array_equal(db.astype(np.float64), bt.grad.numpy())


def test_reference_dz_is_exact_on_exact_inputs():
    """y = -log p for p a power of two is not an fp32 number, but y = 0 and a huge y are: one class with p = 1 and the
    others with exp(-y) = 0 exactly (y = 800).  Then dz = onehot * S - gy in exact arithmetic (gy multiples of 1/64)."""
    rng = np.random.default_rng(3)
    n, C, ncls, Hs, Ws = 2, 21, 19, 3, 5
    hot = rng.integers(0, ncls, (n, Hs, Ws))
    y = np.full((n, C, Hs, Ws), 800.0, np.float32)
    np.put_along_axis(y, hot[:, None], 0.0, axis=1)
    gy = (rng.integers(-64, 65, (n, C, Hs, Ws)) / 64.0).astype(np.float32)
    want = -gy.astype(np.float64)
    S = gy[:, :ncls].astype(np.float64).sum(axis=1)
    np.put_along_axis(want, hot[:, None], (S - np.take_along_axis(gy, hot[:, None], axis=1)[:, 0])[:, None], axis=1)
    want[:, ncls:] = gy[:, ncls:]
    got = hbr.dz(y, gy, ncls)
    assert np.array_equal(got.astype(np.float64), want)
    assert np.array_equal(got[:, ncls:].view(np.uint32), gy[:, ncls:].view(np.uint32))
    assert (hbr.dz_tolerance(y, gy, ncls) > 0).all()


@pytest.mark.parametrize("K, shape, chunk", [(24, (2, 7, 33), 64), (512, (1, 6, 11), 2048)])
def test_reference_stays_within_the_bound_of_autograd(K, shape, chunk):
    """Random inputs with the reference's init: every gradient within hbr.autograd_bounds (a 2^-24 sum |terms| bound,
    derived in its docstring) of torch.autograd's float64 gradients of the same step, and the loss within the bound
    of its own inputs."""
    n, Hs, Ws = shape
    C, ncls = 21, 19
    x, w, b = hr.random_inputs(n, K, Hs, Ws, C, seed=K)
    rng = np.random.default_rng(K + 1)
    target = rng.integers(0, ncls, (n, Hs, Ws))
    target[rng.random((n, Hs, Ws)) < 0.15] = 255
    reg = (rng.standard_normal((n, C - ncls, Hs, Ws)) / 64.0).astype(np.float32)
    loss64, dX64, dW64, db64, z64 = hbr.torch_autograd64(x, w, b, ncls, target, reg)
    loss, dX, dW, db, y, gy, dz = _reference_step(x, w, b, ncls, target, reg, chunk)
    z_mag = np.einsum("ck,nkhw->nchw", np.abs(w.astype(np.float64)), np.abs(x.astype(np.float64)))
    bx, bw, bb = hbr.autograd_bounds(x, w, z_mag, y, gy, dz, ncls, chunk)
    assert (np.abs(dX.astype(np.float64) - dX64) <= bx).all()
    assert (np.abs(dW.astype(np.float64) - dW64) <= bw).all()
    assert (np.abs(db.astype(np.float64) - db64) <= bb).all()
    assert (dX.astype(np.float64) != dX64).any()               # (not vacuous: fp32 does round here)
    # the loss: the mean of y over the valid pixels, each y within ey of the float64 value
    ey = 2 * K * 2.0 ** -24 * z_mag[:, :ncls].max() + 2.0 ** -23 * np.abs(y[:, :ncls]).max() + 2.0 ** -39
    assert abs(loss - loss64) <= ey


def test_nll_edge_cases():
    rng = np.random.default_rng(5)
    n, C, ncls, Hs, Ws = 3, 21, 19, 4, 6
    y = np.abs(rng.standard_normal((n, C, Hs, Ws))).astype(np.float32)
    import torch
    nll = torch.nn.NLLLoss(reduction="mean", ignore_index=255)
    # V = 0: NaN as torch, a zero gradient
    t = np.full((n, Hs, Ws), 255)
    loss, V, bad, g = hbr.nll64(y, t, ncls)
    assert np.isnan(loss) and V == 0 and bad == 0 and not g.any() and g.shape == (n, ncls, Hs, Ws)
    assert torch.isnan(nll(-torch.from_numpy(y[:, :ncls].astype(np.float64)), torch.from_numpy(t)))
    # one frame all ignored: the mean runs over the other frames' pixels
    t = rng.integers(0, ncls, (n, Hs, Ws))
    t[1] = 255
    loss, V, bad, g = hbr.nll64(y, t, ncls)
    yt = torch.from_numpy(y[:, :ncls].astype(np.float64)).requires_grad_(True)
    want = nll(-yt, torch.from_numpy(t))
    want.backward()
    assert V == 2 * Hs * Ws and bad == 0 and abs(loss - want.item()) <= 1e-15 * abs(want.item()) * V
    assert not g[1].any() and np.array_equal(g, yt.grad.numpy().astype(np.float32))
    assert (g.sum(axis=1)[[0, 2]] == np.float32(1.0 / V)).all()
    # a bad target: ignored and counted, negative ones too
    t2 = t.copy()
    t2[0, 0, 0], t2[2, 1, 1] = ncls, -1
    loss2, V2, bad2, g2 = hbr.nll64(y, t2, ncls)
    assert V2 == V - 2 and bad2 == 2 and not g2[0, :, 0, 0].any() and not g2[2, :, 1, 1].any()
    t3 = np.where((t2 < 0) | (t2 >= ncls), 255, t2)
    assert hbr.nll64(y, t3, ncls)[0] == loss2
