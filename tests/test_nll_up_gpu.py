"""The full-resolution semantic NLL through the `up` layer (f16) on the device against tests/nll_up_reference.py.

The kernel's tile writes 7 x 31 cells from 8 x 32 corner blocks, so the shapes are: one cell, 2 x 3 cells, a partial
tile in both directions, exactly one tile and exactly 2 x 2 tiles (whose last block row and column fall on a tile's
ring), 3 x 3 tiles with partial ones, a 13-pixel right margin (which also takes the byte-wise target loads), and 1, 19
and 32 classes in 21, 22 and 40 channels.

The bounds are nll_up_reference.loss_bound and grad_bound, derived there from the kernel's operation sequence with
K_EXP = K_LOG = 3 ulp (the OpenCL C bounds that the device library's expf and logf are built to):
  gradient   1.01 * inv_V * (operator on 21 * 2^-24 |r| + |dr|) + 1024 * 2^-149 per element,
             |dr| = p ((2 K_EXP + |K - u|) 2^-24 + |dK|) + [c == t] |r| 2^-24,
             |dK| = (|K| + 2 K_LOG |log S| + C - 1 + 2 K_EXP + C / e) 2^-24;
  loss       1.01 * (mean (|dK| + |L| 2^-24) + 2^-40 mean |L|) + one fp32 ulp of the loss.
Worst observed fractions of the bound on an MI355X over all cases below, no element excluded: the values that
test_loss_counts_and_gradient_within_the_bound prints are recorded in DESIGN.md 10t (gradient 0.15, loss 0.08)."""
import functools

import numpy as np
import pytest

import cnn_labels_reference as cr
import nll_up_reference as nr
from guards import check_guards
from instance_stixels_amd import core, training

pytestmark = pytest.mark.gpu

GUARD = 64
# name: (n, rows8, cols8, n_classes, channels, margin)
CASES = {
    "1x1": (1, 1, 1, 19, 22, 0),
    "2x3": (2, 2, 3, 19, 22, 0),
    "partial": (2, 5, 20, 19, 22, 0),
    "one_tile": (1, 7, 31, 19, 22, 0),
    "2x2_tiles": (1, 14, 62, 19, 22, 0),
    "3x3_tiles": (2, 16, 65, 19, 22, 0),
    "margin13": (2, 5, 20, 19, 22, 13),
    "1_class": (2, 5, 9, 1, 21, 0),
    "32_classes": (1, 9, 33, 32, 40, 0),
}


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """A case's planes and targets (16 x 16 blocks, 10 % ignored) and its reference, computed once and left unchanged."""
    n, Hs, Ws, ncls, ch, margin = CASES[name]
    seed = 700 + list(CASES).index(name)
    y = cr.random_costs(n, ch, Hs, Ws, seed, n_classes=ncls)
    t = nr.random_targets(n, 8 * Hs, 8 * Ws + margin, ncls, seed + 50)
    if margin:
        t[:, :, 8 * Ws:] = 77                                                # no class: must not count as bad
    y.setflags(write=False)
    t.setflags(write=False)
    return y, t, ncls


@functools.lru_cache(maxsize=None)
def _reference(name):
    y, t, ncls = _inputs(name)
    return nr.evaluate(y, t, ncls)


def _call(y, t, ncls, **kw):
    torch, dev = _torch()
    out = core.semantic_nll_up(torch.tensor(y, device=dev), torch.tensor(t, device=dev), ncls, **kw)
    torch.cuda.synchronize()
    return [o.cpu().numpy() if torch.is_tensor(o) else o for o in out]


def _within_bounds(out, ref, what=""):
    loss, valid, bad, grad = out[:4]
    assert int(valid[0]) == ref["valid"] and int(bad[0]) == ref["bad"]
    lb, gb = nr.loss_bound(ref), nr.grad_bound(ref)
    lf = abs(float(loss[0]) - ref["loss"]) / lb
    gf = float((np.abs(grad.astype(np.float64) - ref["grad"]) / gb).max())
    print(f"{what}: loss {float(loss[0])!r} ref {ref['loss']!r} fraction of the bound {lf:.4f}; gradient {gf:.4f}")
    assert lf < 1 and gf < 1
    return lf, gf


@pytest.mark.parametrize("name", list(CASES))
def test_loss_counts_and_gradient_within_the_bound(name):
    y, t, ncls = _inputs(name)
    ref = _reference(name)
    out = _call(y, t, ncls, canary=GUARD)
    check_guards(out[4], GUARD)
    assert set(out[4]) == {"loss", "valid_count", "bad_count", "grad", "scratch"}
    _within_bounds(out, ref, name)
    assert out[3].shape == ref["grad"].shape and np.isfinite(out[3]).all()


@pytest.mark.parametrize("name", ["partial", "3x3_tiles", "margin13"])
def test_two_runs_and_the_loss_only_call_agree_bit_for_bit(name):
    y, t, ncls = _inputs(name)
    a, b = _call(y, t, ncls), _call(y, t, ncls)
    for u, v in zip(a, b):
        assert np.array_equal(_bits(u), _bits(v))
    only = _call(y, t, ncls, grad=False, canary=GUARD)
    check_guards(only[4], GUARD)
    assert only[3] is None and set(only[4]) == {"loss", "valid_count", "bad_count", "scratch"}
    for u, v in zip(a[:3], only[:3]):
        assert np.array_equal(_bits(u), _bits(v))


def test_a_frame_keeps_its_gradient_in_another_batch_position():
    y, t, ncls = _inputs("3x3_tiles")
    a = _call(y, t, ncls)
    b = _call(y[::-1].copy(), t[::-1].copy(), ncls)
    assert int(a[1][0]) == int(b[1][0])
    assert np.array_equal(_bits(a[3]), _bits(b[3][::-1]))


@pytest.mark.parametrize("name", ["2x3", "3x3_tiles"])
def test_a_batch_of_one_frame_twice_halves_the_gradient_exactly(name):
    """inv_V halves exactly, and the sums behind it do not see the batch (the costs are far from the subnormals)."""
    y, t, ncls = _inputs(name)
    one = _call(y[:1], t[:1], ncls)
    two = _call(np.concatenate((y[:1], y[:1])), np.concatenate((t[:1], t[:1])), ncls)
    assert np.array_equal(_bits(one[0]), _bits(two[0])) and int(two[1][0]) == 2 * int(one[1][0])
    half = one[3] * np.float32(0.5)
    assert np.abs(one[3][one[3] != 0]).min() > 2.0 ** -100
    assert np.array_equal(_bits(two[3][0]), _bits(half[0])) and np.array_equal(_bits(two[3][1]), _bits(half[0]))


def test_ignored_pixels_at_tile_borders_in_whole_tiles_and_a_whole_frame():
    """Cells 6..8 x 29..33 straddle the tiles' rings; cells 7..13 x 31..61 are one whole tile; frame 1 is ignored
    altogether and must get an all-zero gradient inside a batch that has valid frames."""
    y, t, ncls = _inputs("3x3_tiles")
    y = np.concatenate((y, y[:1]))
    t = np.concatenate((t, t[:1])).copy()
    t[0, 8 * 6 - 3:8 * 9 + 2, 8 * 29 + 5:8 * 34 - 1] = 255
    t[2, 8 * 7:8 * 14, 8 * 31:8 * 62] = 255
    t[1] = 255
    ref = nr.evaluate(y, t, ncls)
    out = _call(y, t, ncls, canary=GUARD)
    check_guards(out[4], GUARD)
    _within_bounds(out, ref, "ignored")
    assert not _bits(out[3][1]).any()                                        # +0.0f everywhere
    assert not out[3][2, :, 8:13, 32:61].any() and out[3][2, :, 7, 31].any()  # cells no valid pixel reaches


def test_no_valid_pixel_gives_nan_and_zeros_and_bad_targets_are_counted():
    torch, dev = _torch()
    y, t, ncls = _inputs("partial")
    out = _call(y, np.full_like(t, 255), ncls, canary=GUARD)
    check_guards(out[4], GUARD)
    assert np.isnan(out[0][0]) and int(out[1][0]) == 0 and int(out[2][0]) == 0 and not _bits(out[3]).any()
    k = int(t[0, 0, 0])
    t2 = np.where(t == k, 19, t)                                             # 19: a channel, but no class
    ref = nr.evaluate(y, t2, ncls)
    assert ref["bad"] > 0
    _within_bounds(_call(y, t2, ncls, check=False), ref, "bad targets")
    with pytest.raises(core.CoreError, match=f"{ref['bad']} targets are neither a class"):
        core.semantic_nll_up(torch.tensor(y, device=dev), torch.tensor(t2, device=dev), ncls)
    own = _call(y, t, ncls, ignore_index=k, check=False)                     # an ignore_index that is a class id:
    good = _call(y, np.where(t == 255, k, t), ncls, ignore_index=k)          # 255 is then a bad target like any other
    assert int(own[2][0]) == int((t == 255).sum()) > 0 and int(good[2][0]) == 0
    for u, v in zip(own[:2] + own[3:4], good[:2] + good[3:4]):
        assert np.array_equal(_bits(u), _bits(v))
    assert int(own[1][0]) == int(((t != 255) & (t != k)).sum())


def test_a_wider_gradient_tensor_keeps_the_planes_behind():
    torch, dev = _torch()
    y, t, ncls = _inputs("margin13")
    n, ch, Hs, Ws = y.shape
    fresh = _call(y, t, ncls)
    gy = torch.full((n, ch + 1, Hs, Ws), -7.0, device=dev)
    out = core.semantic_nll_up(torch.tensor(y, device=dev), torch.tensor(t, device=dev), ncls, grad=gy)
    assert out[3] is gy
    got = gy.cpu().numpy()
    assert np.array_equal(_bits(got[:, :ncls]), _bits(fresh[3])) and (got[:, ncls:] == -7.0).all()
    assert np.array_equal(_bits(out[0].cpu().numpy()), _bits(fresh[0]))


def test_class_and_regression_planes_of_one_gradient_tensor_are_each_written_once():
    """semantic_nll_up on the class planes and is_offset_loss on the regression planes of one gy: every plane equals
    what the separate calls give, so none is written twice or left unwritten (the tensor starts as NaN)."""
    torch, dev = _torch()
    y, t, ncls = _inputs("partial")
    n, ch, Hs, Ws = y.shape
    nreg, P = 2, Hs * Ws
    yd = torch.tensor(y[:, :ncls + nreg], device=dev).contiguous()
    ids = np.random.default_rng(5).choice(np.array([0, 5, 26, 255, 1001, 1002, 26001], np.int32), (n, Hs, Ws))
    ids8 = torch.tensor(ids, device=dev)
    gy = torch.full((n, ncls + nreg, Hs, Ws), float("nan"), device=dev)
    out = core.semantic_nll_up(yd, torch.tensor(t, device=dev), ncls, grad=gy)
    nbytes = core.offset_loss_scratch_bytes(n, nreg, Hs, Ws)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    loss5 = torch.empty(5, device=dev)
    rc = core.offset_loss_ptr(
        torch.cuda.current_stream(dev).cuda_stream, d_prediction=yd.data_ptr() + 4 * ncls * P,
        prediction_image_stride=(ncls + nreg) * P, d_ids8=ids8.data_ptr(), n_images=n, planes=nreg, rows8=Hs, cols8=Ws,
        w_offset_mean=1e-3, w_offset_variance=1e-4, d_loss=loss5.data_ptr(), d_grad=gy.data_ptr() + 4 * ncls * P,
        grad_image_stride=(ncls + nreg) * P, d_scratch=scratch.data_ptr(), scratch_bytes=nbytes)
    assert rc == 0, core.lib().is_last_error()
    torch.cuda.synchronize()
    g_cls = _call(y, t, ncls)[3]
    g_reg = core.offset_loss(yd[:, ncls:], ids8, None, weights=(1e-3, 1e-4, 0.0, 0.0))[2].cpu().numpy()
    got = gy.cpu().numpy()
    assert np.array_equal(_bits(got[:, :ncls]), _bits(g_cls)) and np.array_equal(_bits(got[:, ncls:]), _bits(g_reg))
    assert out[3] is gy


def test_training_step_equals_the_direct_calls(monkeypatch):
    """SegmentationHead -> SemanticNLLLossUp -> backward(): one call of each, and weight.grad, bias.grad and the
    feature gradient are bit for bit core.segmentation_head_backward of core.semantic_nll_up's gradient."""
    import head_reference as hr
    torch, dev = _torch()
    n, K, Hs, Ws, ncls, nreg = 2, 24, 9, 33, 19, 2
    x, w, b = hr.random_inputs(n, K, Hs, Ws, ncls + nreg, seed=31)
    t = torch.tensor(nr.random_targets(n, 8 * Hs, 8 * Ws, ncls, 32), device=dev)
    head = training.SegmentationHead(K, ncls, nreg).to(dev)
    head.load_state_dict({"weight": torch.tensor(w).reshape(ncls + nreg, K, 1, 1), "bias": torch.tensor(b)})
    calls, losses = [], []
    real_b, real_l = core.segmentation_head_backward, core.semantic_nll_up
    monkeypatch.setattr(core, "segmentation_head_backward", lambda *a, **kw: calls.append(kw) or real_b(*a, **kw))
    monkeypatch.setattr(core, "semantic_nll_up", lambda *a, **kw: losses.append(kw) or real_l(*a, **kw))
    features = torch.tensor(x, device=dev, requires_grad=True)
    out = head(features)
    loss = training.SemanticNLLLossUp(n_classes=ncls)(out, t[:, None].to(torch.int64))
    loss.backward()
    assert len(calls) == 1 and len(losses) == 1
    assert calls[0]["want_features"] and calls[0]["want_weight"] and calls[0]["want_bias"]

    y = core.segmentation_head(features.detach(), w, b, ncls, 1 << int(Hs).bit_length(), want_segmentation=False)
    assert np.array_equal(_bits(out.detach().cpu().numpy()), _bits(y.cpu().numpy()))
    gy = torch.zeros_like(y)                                                 # (the regression planes get no gradient)
    l_cls = real_l(y, t, ncls, grad=gy)[0]
    assert np.array_equal(_bits(loss.detach().cpu().numpy()), _bits(l_cls[0].cpu().numpy()))
    g = real_b(features.detach(), head.weight.detach(), y, gy, ncls)
    assert np.array_equal(_bits(features.grad.cpu().numpy()), _bits(g["features"].cpu().numpy()))
    assert np.array_equal(_bits(head.weight.grad.cpu().numpy().reshape(-1, K)), _bits(g["weight"].cpu().numpy()))
    assert np.array_equal(_bits(head.bias.grad.cpu().numpy()), _bits(g["bias"].cpu().numpy()))
    assert float(head.weight.grad.abs().max()) > 0
