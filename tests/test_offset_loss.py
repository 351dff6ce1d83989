"""CPU tests of f12 (offset and disparity training losses): the numpy restatement of tests/offset_loss_reference.py
against the reference's own classes run in float64 (tests/golden/reference_python_losses), the surface of the new entry
points (declared, exported, bound) and the refusals that need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import offset_loss_reference as lr
from instance_stixels_amd import core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_python_losses", "offset_losses_reference_python.npz")
CORE_SYMBOLS = ["is_offset_loss_scratch_bytes", "is_offset_loss"]
FAKE = 0x10000   # a "device pointer" that is never dereferenced: every call below is refused before any device call
RTOL = 1e-10     # both sides are binary64 with another order of summation; n * 2^-53 is far below


def fixture():
    z = np.load(GOLDEN)
    names = bytes(z["names"]).decode().split(",")
    return z, names, tuple(z["weights"].tolist())


def case(z, name):
    return z[f"{name}_pred"], z[f"{name}_ids"], z[f"{name}_d8"]


def close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f"{what}: nan where the reference has none")
    ok = ~np.isnan(want)
    np.testing.assert_allclose(got[ok], want[ok], rtol=RTOL, atol=0, err_msg=what)
    assert (got[ok][want[ok] == 0] == 0).all(), f"{what}: an exact zero is not exact"


def test_fixture_holds_every_corner_case():
    z, names, weights = fixture()
    stat_names = bytes(z["stat_names"]).decode().split(",")
    assert {"zero_stuff", "zero_pos_g", "zero_disp_med", "equal_pos", "n1", "n2", "n3", "id10", "id11", "id255", "id1000",
            "id1001", "negative_id", "two_parts", "no_disparity", "even_median", "no_keys", "no_stuff",
            "keys65"} <= set(stat_names)
    assert (z["stats"] >= 1).all(), dict(zip(stat_names, z["stats"].tolist()))
    assert set(names) == {"general", "no_keys", "no_stuff", "many_keys", "tiny"}
    assert all(np.float32(w) == w for w in weights), "the weights must be exact in float32"
    assert z["general_pred"].shape == (3, 24, 50) and lr.key_counts(z["many_keys_ids"][None])[0] >= 65
    five = z["no_stuff_d_D0_five"]
    assert np.isnan(five[[0, 1, 3]]).all() and np.isfinite(five[[2, 4]]).all()
    assert np.isfinite(z["no_stuff_d_D0_grad"]).all()
    # no sign argument in (0, guard): the restatement's own arguments, both settings
    for name in names:
        for a in (False, True):
            args = {}
            lr.frame(*case(z, name), weights, a, sign_args=args)
            v = np.abs(np.concatenate([np.asarray(x, np.float64) for x in args.values()]))
            assert not ((v > 0) & (v < float(z["guard"]))).any(), (name, a)


@pytest.mark.parametrize("name", ["general", "no_keys", "no_stuff", "many_keys", "tiny"])
@pytest.mark.parametrize("abs_variance", [0, 1])
def test_restatement_equals_the_reference_in_float64(name, abs_variance):
    z, _, weights = fixture()
    pred, ids, d8 = case(z, name)
    five, terms, grad = lr.batch(pred[None], ids[None], d8[None], weights, bool(abs_variance))
    ref = f"{name}_d_D{abs_variance}"
    close(five, z[f"{ref}_five"], "five")
    close(five[0], z[f"{ref}_loss"], "loss")
    close(terms[0], z[f"{ref}_five"][1:], "terms")
    close(grad[0], z[f"{ref}_grad"], "gradient")
    # OffsetLossSL: the two offset planes; it has no abs_variance (its **kwargs swallow the keyword)
    five2, terms2, grad2 = lr.batch(pred[None, 1:], ids[None], None, weights, False)
    close(five2[0], z[f"{name}_d_O{abs_variance}_loss"], "OffsetLossSL loss")
    close(grad2[0], z[f"{name}_d_O{abs_variance}_grad"], "OffsetLossSL gradient")
    close(terms2[0, :2], z[f"{name}_d_D0_five"][1:3], "the offset terms of both classes")
    assert (terms2[0, 2:] == 0).all() and (five2[3:] == 0).all()


def test_restatement_weights_batches_and_the_torch_loop():
    """A zero weight removes its lines of the gradient; a batch sums the frames' terms; the torch loop (the timing
    yardstick) in float64 with autograd equals the closed form."""
    import torch
    z, _, weights = fixture()
    pred, ids, d8 = case(z, "general")
    full = lr.frame(pred, ids, d8, weights, False)[1]
    parts = np.zeros_like(full)
    for k in range(4):
        w = [0.0] * 4
        w[k] = weights[k]
        terms, g = lr.frame(pred, ids, d8, w, False)
        parts += g
        assert np.isfinite(g).all()
    np.testing.assert_allclose(parts, full, rtol=1e-12, atol=1e-18)
    p2 = np.stack([pred, pred[:, ::-1].copy()])
    i2, dd = np.stack([ids, ids[::-1]]), np.stack([d8, d8[::-1]])
    for a in (False, True):
        five, terms, grad = lr.batch(p2, i2, dd, weights, a)
        close(five[1:], terms[0] + terms[1], "batch sums")
        p = torch.from_numpy(p2.astype(np.float64)).requires_grad_(True)
        loss, sums = lr.torch_loop_loss(p, torch.from_numpy(i2.astype(np.int64)),
                                        torch.from_numpy((dd.astype(np.int64) >> 8).astype(np.float64)), weights, a)
        close(five[0], loss.item(), "torch loop loss")
        close(five[1:], [float(s.detach()) for s in sums], "torch loop sums")
        close(grad, torch.autograd.grad(loss, p)[0].numpy(), "torch loop gradient")
    assert lr.ulp_distance(np.float32(1) + np.spacing(np.float32(1)), 1.0) == 1.0
    assert lr.ulp_distance(np.float32(np.nan), np.nan) == 0 and np.isinf(lr.ulp_distance(np.float32(1e-30), 0.0))


def test_symbols_are_declared_exported_and_bound(tmp_path):
    text = open(os.path.join(ROOT, "include", "instance_stixels_core.h")).read()
    declared = set(re.findall(r"\b(is_[a-z0-9_]+)\s*\(", text))
    L = core.lib()
    for name in CORE_SYMBOLS:
        assert name in declared, f"{name} is not declared in instance_stixels_core.h"
        assert name in core.EXPORTS
        assert hasattr(L, name), f"libis_core.so does not export {name}"
    for name in ("OffsetLossArgs", "offset_loss_scratch_bytes", "offset_loss_ptr", "offset_loss"):
        assert hasattr(core, name)
    from instance_stixels_amd import training
    assert hasattr(training, "OffsetLossSL") and hasattr(training, "DisparityOffsetLossSL")
    # the struct of the binding has the size and the offsets the header's declaration gives on this ABI
    fields = [f[0] for f in core.OffsetLossArgs._fields_]
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "instance_stixels_core.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(is_offset_loss_args));\n'
                   + "".join(f'  printf(" %zu", offsetof(is_offset_loss_args, {f}));\n' for f in fields)
                   + "  return 0;\n}\n")
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == ctypes.sizeof(core.OffsetLossArgs) == 136
    assert got[1:] == [getattr(core.OffsetLossArgs, f).offset for f in fields]


def _refused(match, **fields):
    base = dict(d_prediction=FAKE, prediction_image_stride=3 * 16 * 32, d_ids8=FAKE, d_disparity8_u16=FAKE, n_images=1,
                planes=3, rows8=16, cols8=32, d_loss=FAKE, d_scratch=FAKE, scratch_bytes=1 << 40)
    base.update(fields)
    assert core.offset_loss_ptr(**base) == -1, fields
    err = core.lib().is_last_error().decode()
    assert "invalid argument" in err and re.search(match, err), (fields, err)


def test_offset_loss_refuses_bad_arguments_without_a_gpu():
    assert core.lib().is_offset_loss(None, None) == -1
    _refused("null d_prediction", d_prediction=None)
    _refused("null d_ids8", d_ids8=None)
    _refused("null d_loss", d_loss=None)
    _refused("null d_scratch", d_scratch=None)
    for planes in (0, 1, 4, -2):
        _refused("planes", planes=planes)
    _refused("d_disparity8_u16", d_disparity8_u16=None)                                    # 3 planes without it
    _refused("d_disparity8_u16", planes=2, prediction_image_stride=2 * 16 * 32)            # 2 planes with it
    for rows8, cols8 in ((0, 32), (16, 0), (-1, 32), (16, -4)):
        _refused("positive", rows8=rows8, cols8=cols8)
    _refused("2\\^28", rows8=1 << 14, cols8=(1 << 14) + 1, prediction_image_stride=1 << 40)
    _refused("prediction_image_stride", prediction_image_stride=3 * 16 * 32 - 1)
    _refused("prediction_image_stride", prediction_image_stride=0)
    _refused("grad_image_stride", d_grad=FAKE, grad_image_stride=3 * 16 * 32 - 1)
    _refused("n_images", n_images=0)
    _refused("n_images", n_images=65536)
    _refused("capacity", capacity=-1)
    _refused("capacity", capacity=16 * 32 + 1)                                             # more rows than cells
    _refused("capacity", capacity=8193, rows8=128, cols8=256, prediction_image_stride=3 * 128 * 256)
    _refused("16-byte aligned", d_scratch=FAKE + 8)
    _refused("4-byte aligned", d_prediction=FAKE + 2)
    _refused("4-byte aligned", d_grad=FAKE + 1, grad_image_stride=3 * 16 * 32)
    _refused("4-byte aligned", d_key_count=FAKE + 2)
    _refused("2-byte aligned", d_disparity8_u16=FAKE + 1)
    need = core.offset_loss_scratch_bytes(1, 3, 16, 32, 0)
    assert need > 0 and need % 16 == 0
    _refused("scratch_bytes", scratch_bytes=need - 1)
    _refused("scratch_bytes", scratch_bytes=core.offset_loss_scratch_bytes(1, 2, 16, 32, 0))  # the histograms need more


def test_scratch_query_refuses_what_the_call_refuses():
    q = core.offset_loss_scratch_bytes
    assert q(0, 3, 16, 32) == 0 and q(65536, 3, 16, 32) == 0 and q(1, 1, 16, 32) == 0 and q(1, 4, 16, 32) == 0
    assert q(1, 3, 0, 32) == 0 and q(1, 3, 16, -1) == 0 and q(1, 3, 1 << 14, (1 << 14) + 1) == 0
    assert q(1, 3, 16, 32, 513) == 0 and q(1, 3, 16, 32, -1) == 0 and q(1, 3, 128, 256, 8193) == 0
    assert q(1, 3, 16, 32, 256) == q(1, 3, 16, 32, 0) > q(1, 2, 16, 32, 0) > 0                # 0: min(256, cells)
    assert q(1, 3, 2, 3, 6) == q(1, 3, 2, 3, 0) > 0
    assert q(2, 3, 128, 256) > q(1, 3, 128, 256) > q(1, 3, 128, 256, 64) > 0
