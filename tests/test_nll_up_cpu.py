"""The full-resolution semantic NLL through the `up` layer (f16) without a GPU: the symbols and bindings, the struct
layout, every refusal of is_semantic_nll_up (all made before the device is touched), the reference of
tests/nll_up_reference.py pinned against torch in float64, the linearity claim the feature rests on, and the cases
with exact arithmetic."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cnn_labels_reference as cr
import nll_up_reference as nr
from instance_stixels_amd import core, training

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "instance_stixels_core.h")).read()
    for name in ("is_semantic_nll_up", "is_semantic_nll_up_scratch_bytes"):
        assert name + "(" in header
        assert name in core.EXPORTS and hasattr(core.lib(), name), name
    assert callable(core.semantic_nll_up) and callable(core.semantic_nll_up_ptr)
    assert callable(core.semantic_nll_up_scratch_bytes) and callable(training.SemanticNLLLossUp)
    for cite in ("DRNSeg.py:46-225", "train.py:69-232"):
        assert cite in header, cite
    kernels = os.path.join(ROOT, "instance_stixels_amd", "csrc")
    for name in ("is_k_cnn_labels.hip", "is_k_nll_up.hip"):                  # one copy of the weights
        text = open(os.path.join(kernels, name)).read()
        assert '#include "is_cnn_up.h"' in text and "float cnn_w_low(" not in text, name


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "instance_stixels_core.h"
#define F(f) printf(#f " %zu %zu\n", offsetof(is_semantic_nll_up_args, f), sizeof(((is_semantic_nll_up_args*)0)->f));
int main() {
    printf(". %zu 0\n", sizeof(is_semantic_nll_up_args));
    FIELDS
    return 0;
}
"""


def test_args_layout_matches_the_header(tmp_path):
    src = PROBE.replace("FIELDS", "".join(f"F({n})" for n, _ in core.SemanticNllUpArgs._fields_))
    (tmp_path / "probe.cpp").write_text(src)
    exe = str(tmp_path / "probe")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "probe.cpp"), "-o", exe],
                   check=True)
    got = {f: (int(off), int(size)) for f, off, size in
           (l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())}
    assert got["."][0] == ctypes.sizeof(core.SemanticNllUpArgs)
    for name, _ in core.SemanticNllUpArgs._fields_:
        field = getattr(core.SemanticNllUpArgs, name)
        assert got[name] == (field.offset, field.size), name


# A call that would be accepted (the pointers are never dereferenced on the host: every case below is refused before
# the device is touched, so this file needs no GPU).
PLANES = 19 * 5 * 7
GOOD = dict(d_cnn_out=0x1000, cnn_image_stride=21 * 5 * 7, d_target=0x2001, ignore_index=255, n_images=2, rows8=5,
            cols8=7, n_classes=19, mode=core.CNN_UP_DECONV, rows=40, cols=56, d_loss=0x3000, d_valid_count=0x4000,
            d_bad_count=0x5000, d_grad=0x6000, grad_image_stride=PLANES, d_scratch=0x7000, scratch_bytes=1 << 20)


@pytest.mark.parametrize("change, message", [
    (dict(d_cnn_out=None), "null d_cnn_out"),
    (dict(d_target=None), "null d_cnn_out or d_target"),
    (dict(d_loss=None), "null d_loss"),
    (dict(d_valid_count=None), "d_valid_count"),
    (dict(d_bad_count=None), "d_bad_count"),
    (dict(d_loss=None, d_valid_count=None, d_bad_count=None, d_grad=None), "null d_loss"),   # every output
    (dict(mode=core.CNN_UP_NEAREST), "1/8 resolution is is_semantic_nll"),
    (dict(mode=2), "mode"),
    (dict(mode=-1), "mode"),
    (dict(rows=41), "8 \\* rows8"),
    (dict(rows=32), "8 \\* rows8"),
    (dict(cols=55), "8 \\* cols8"),
    (dict(rows8=0, rows=0), "rows8"),
    (dict(cols8=0), "cols8"),
    (dict(n_classes=0), "n_classes"),
    (dict(n_classes=33), "IS_HEAD_MAX_CHANNELS"),
    (dict(n_images=0), "n_images"),
    (dict(n_images=65536), "n_images"),
    (dict(cnn_image_stride=PLANES - 1), "cnn_image_stride"),
    (dict(grad_image_stride=PLANES - 1), "grad_image_stride"),
    (dict(rows8=8192, rows=65536, cols8=4096, cols=32768, n_classes=1, cnn_image_stride=1 << 40,
          grad_image_stride=1 << 40), "rows \\* cols"),                                        # 2^31 pixels
    (dict(rows8=2048, rows=16384, cols8=8192, cols=65536 + 65536, n_classes=1, cnn_image_stride=1 << 40,
          grad_image_stride=1 << 40), "rows \\* cols"),                      # the margin takes rows * cols to 2^31
    (dict(d_cnn_out=0x1002), "4-byte aligned"),
    (dict(d_loss=0x3002), "4-byte aligned"),
    (dict(d_grad=0x6001), "4-byte aligned"),
    (dict(d_valid_count=0x4004), "8-byte aligned"),
    (dict(d_bad_count=0x5004), "8-byte aligned"),
    (dict(d_scratch=None), "null d_scratch"),
    (dict(d_scratch=0x7008), "d_scratch must be 16-byte aligned"),
    (dict(scratch_bytes=15), "scratch_bytes"),
    (dict(reserved=(0, 0, 1, 0)), "reserved"),
])
def test_refusals_need_no_device(change, message):
    rc = core.semantic_nll_up_ptr(**dict(GOOD, **change))
    assert rc == -1                                                          # IS_EINVAL
    assert re.search(message, core.lib().is_last_error().decode()), core.lib().is_last_error()


def test_null_args_are_refused():
    assert core.lib().is_semantic_nll_up(None, None) == -1
    assert b"null args" in core.lib().is_last_error()


def test_scratch_bytes_is_zero_for_a_refused_shape_and_exact_for_a_good_one():
    f = core.semantic_nll_up_scratch_bytes
    for bad in ((0, 5, 7, 19), (65536, 5, 7, 19), (1, 0, 7, 19), (1, 5, 0, 19), (1, 5, 7, 0), (1, 5, 7, 33),
                (1, 8192, 4096, 1)):
        assert f(*bad) == 0, bad
    assert f(2, 5, 7, 19) > 0 and f(4, 5, 7, 19) == 2 * f(2, 5, 7, 19)
    assert core.semantic_nll_up_ptr(**dict(GOOD, scratch_bytes=f(2, 5, 7, 19) - 1)) == -1
    assert b"scratch_bytes" in core.lib().is_last_error()


def test_module_refuses_targets_that_are_no_class_ids():
    import torch
    loss = training.SemanticNLLLossUp()
    out = torch.zeros((1, 19, 1, 1))
    with pytest.raises(core.CoreError, match="integer class ids"):
        loss(out, torch.zeros((1, 8, 8)))
    with pytest.raises(core.CoreError, match=r"outside \[0, 255\]"):
        loss(out, torch.full((1, 8, 8), 256, dtype=torch.int32))
    with pytest.raises(core.CoreError, match=r"outside \[0, 255\]"):
        loss(out, torch.full((1, 1, 8, 8), -1, dtype=torch.int64))


# ---- the reference against torch in float64 ----

def _w64(C):
    import torch
    w1 = torch.from_numpy(cr.weights().astype(np.float64))
    return (w1[:, None] * w1[None, :]).expand(C, 1, 16, 16).contiguous()


def _torch_loss64(planes, target, ignore_index=255, logits=False):
    """nll_loss(log_softmax(conv_transpose2d(-y))) in float64 (of the logits themselves with logits=True) and its
    autograd gradient with respect to the planes."""
    import torch
    import torch.nn.functional as F
    x = torch.tensor(np.asarray(planes, np.float64), requires_grad=True)
    C = x.shape[1]
    up = F.conv_transpose2d(x if logits else -x, _w64(C), stride=8, padding=4, groups=C)
    Wd = up.shape[-1]
    t = torch.tensor(np.asarray(target)[:, :, :Wd].astype(np.int64))
    loss = F.nll_loss(F.log_softmax(up, dim=1), t, ignore_index=ignore_index)
    loss.backward()
    return float(loss.detach()), x.grad.numpy()


def _up_abs64(planes):
    import torch
    import torch.nn.functional as F
    x = torch.tensor(np.abs(np.asarray(planes, np.float64)))
    return F.conv_transpose2d(x, _w64(x.shape[1]), stride=8, padding=4, groups=x.shape[1]).numpy()


def test_operator_is_the_transposed_convolution():
    rng = np.random.default_rng(3)
    v = rng.standard_normal((2, 3, 4, 5))
    import torch
    import torch.nn.functional as F
    want = F.conv_transpose2d(torch.tensor(v), _w64(3), stride=8, padding=4, groups=3).numpy()
    got = np.einsum("iy,ncij,jx->ncyx", nr.operator(4), v, nr.operator(5))
    assert np.abs(got - want).max() < 1e-13
    r = rng.standard_normal((2, 3, 32, 40))
    assert abs((nr.transposed(r) * v).sum() - (r * want).sum()) < 1e-10      # <A r, v> == <r, A^T v>


@pytest.mark.parametrize("Hs, Ws, C, margin, seed", [(5, 7, 19, 0, 21), (3, 4, 19, 13, 22), (1, 1, 5, 0, 23),
                                                      (9, 2, 32, 0, 24)])
def test_reference_equals_torch_within_what_the_fp32_chain_allows(Hs, Ws, C, margin, seed):
    """The reference works on the fp32 chain values, torch on exact ones: |du| <= B = 4 * 2^-24 * sum w |v| per pixel
    and class (test_cnn_labels_cpu.py).  The pixel loss u_t + logsumexp(-u) moves by at most 2 max_c B, a softmax
    probability by at most 2 p max_c B; the operator passes the second on to the gradient."""
    y = cr.random_costs(2, C + 2, Hs, Ws, seed, n_classes=C)
    t = nr.random_targets(2, 8 * Hs, 8 * Ws + margin, C, seed + 100, ignored=0.2, block=4)
    ref = nr.evaluate(y, t, C)
    loss64, grad64 = _torch_loss64(y[:, :C], t)
    B = (4 * 2.0 ** -24 * _up_abs64(y[:, :C])).max(axis=1)
    counts = ref["counts"]
    assert 0 < ref["valid"] < counts.size and ref["bad"] == 0
    loss_tol = 2 * (B * counts).sum() / ref["valid"] + 1e-13
    print("loss", ref["loss"], loss64, "err / bound", abs(ref["loss"] - loss64) / loss_tol)
    assert abs(ref["loss"] - loss64) <= loss_tol
    grad_tol = nr.transposed(2 * ref["p"] * (B * counts)[:, None]) / ref["valid"] + 1e-15
    err = np.abs(ref["grad"] - grad64)
    print("grad err / bound", float((err / grad_tol).max()))
    assert (err <= grad_tol).all() and err.max() > 0
    assert np.abs(ref["grad"].sum(axis=1)).max() < 1e-12                     # the class sum of a cell is zero


@pytest.mark.parametrize("Hs, Ws", [(1, 1), (2, 3), (4, 5)])
def test_linearity_the_cost_planes_carry_the_loss_of_the_logits(Hs, Ws):
    """With y = -log_softmax(z) in float64: the loss of up(y) IS nll_loss(log_softmax(up(z))), border cells and a
    one-cell plane included, and the gradient with respect to y, pushed through the head's Jacobian
    dz_j = exp(-y_j) sum_c g_c - g_j, IS autograd's dL/dz."""
    rng = np.random.default_rng(40 + Hs)
    C = 7
    z = 3.0 * rng.standard_normal((2, C, Hs, Ws))
    zmax = z.max(axis=1, keepdims=True)
    y = (zmax + np.log(np.exp(z - zmax).sum(axis=1, keepdims=True))) - z
    t = nr.random_targets(2, 8 * Hs, 8 * Ws, C, 50 + Hs, ignored=0.2, block=2)
    u = np.einsum("iy,ncij,jx->ncyx", nr.operator(Hs), y, nr.operator(Ws))
    ref = nr.from_values(u, t)
    loss_z, grad_z = _torch_loss64(z, t, logits=True)
    assert abs(ref["loss"] - loss_z) < 1e-12
    g = ref["grad"]
    dz = np.exp(-y) * g.sum(axis=1, keepdims=True) - g
    assert np.abs(dz - grad_z).max() < 1e-12
    assert np.abs(g.sum(axis=1)).max() < 1e-12


def test_one_class_of_dyadic_planes_has_loss_and_gradient_exactly_zero():
    rng = np.random.default_rng(6)
    y = (rng.integers(0, 256, (2, 3, 4, 5)) / 8.0).astype(np.float32)
    t = np.zeros((2, 32, 40), np.uint8)
    ref = nr.evaluate(y, t, 1)
    assert ref["loss"] == 0.0 and ref["valid"] == t.size and ref["bad"] == 0
    assert not ref["pixel_loss"].any() and not ref["grad"].any()


def test_all_targets_ignored_give_nan_and_zeros():
    y = cr.random_costs(1, 19, 2, 3, 7)
    ref = nr.evaluate(y, np.full((1, 16, 24), 255, np.uint8), 19)
    assert np.isnan(ref["loss"]) and ref["valid"] == 0 and ref["bad"] == 0 and not ref["grad"].any()


def test_targets_beyond_the_classes_are_bad_and_ignored():
    y = cr.random_costs(1, 21, 2, 3, 8)
    t = nr.random_targets(1, 16, 24 + 5, 19, 9, ignored=0.0, block=4)
    k = int(t[0, 0, 0])                                                      # a class that does occur
    good = nr.evaluate(y, np.where(t == k, 255, t), 19)
    t2 = np.where(t == k, 19, t)                                             # 19: a channel, but no class
    t2[:, :, 24:] = 200                                                      # the margin takes no part
    ref = nr.evaluate(y, t2, 19)
    assert ref["bad"] == int((t[:, :, :24] == k).sum()) > 0 and ref["valid"] == good["valid"]
    assert ref["loss"] == good["loss"] and np.array_equal(ref["grad"], good["grad"])
    own = nr.evaluate(y, t, 19, ignore_index=k)                              # an ignore_index that is a class id
    assert own["bad"] == 0 and own["loss"] == good["loss"] and np.array_equal(own["grad"], good["grad"])
