"""The head's backward pass and the semantic NLL loss (f14) on the device against tests/head_backward_reference.py.
Two-stage, as f13's tests: dz against float64 within the contract's bound, then dX, dW and db bit for bit as the
reference's chains evaluated on the device's OWN dz (d_grad_logits).  y comes from a real core.segmentation_head call."""
import functools

import numpy as np
import pytest

import head_backward_reference as hbr
import head_reference as hr
from guards import check_guards
from instance_stixels_amd import core, training

pytestmark = pytest.mark.gpu

T = core.HEAD_BACKWARD_CHUNK
# (n, K, rows8, cols8)
SHAPES = [
    (1, 8, 5, 7),             # smaller than any tile
    (3, 24, 7, 33),           # ragged tiles, K that is not a multiple of 16
    (2, 512, 16, 40),         # the real K
    (1, 512, 98, 224),        # the reference's operating point
    (1, 8, T // 64, 64),      # P = T exactly
    (2, 40, 1, 2 * T + 37),   # a short last chunk, a second k-tile of 8 features
]
SPLITS = [(19, 2), (19, 3), (19, 0), (30, 2)]
CASES = [(s, 0) for s in range(len(SHAPES))] + [(1, k) for k in range(1, len(SPLITS))]
IDS = ["%dx%dx%dx%d-%d+%d" % (SHAPES[s] + SPLITS[k]) for s, k in CASES]
SMALL = [(0, 0), (1, 0), (1, 3), (5, 0)]
SMALL_IDS = [IDS[CASES.index(c)] for c in SMALL]
GUARD = 64


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _np(t):
    import torch
    return (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _inputs(s, k):
    """A case's inputs, computed once and left unchanged: random features and weights, y from the device's own
    forward, a random gy with exact zeros and one frame (the first row of a single frame) whose class planes are all
    zero."""
    torch, dev = _torch()
    n, K, Hs, Ws = SHAPES[s]
    ncls, nreg = SPLITS[k]
    x, w, b = hr.random_inputs(n, K, Hs, Ws, ncls + nreg, seed=300 + 10 * s + k)
    y = core.segmentation_head(torch.tensor(x, device=dev), w, b, ncls, 1 << int(Hs).bit_length(),
                               want_segmentation=False).cpu().numpy()
    gy = hbr.random_grad(y.shape, ncls, seed=400 + 10 * s + k)
    for a in (x, w, y, gy):
        a.setflags(write=False)
    return dict(x=x, w=w, y=y, gy=gy, ncls=ncls)


def _call(c, x=None, frames=slice(None), **kw):
    torch, dev = _torch()
    x = torch.tensor(c["x"][frames], device=dev) if x is None else x
    out = core.segmentation_head_backward(x, torch.tensor(c["w"], device=dev), torch.tensor(c["y"][frames], device=dev),
                                          torch.tensor(c["gy"][frames], device=dev), c["ncls"], **kw)
    return {name: (v if name == "guards" else _np(v)) for name, v in out.items()}


@functools.lru_cache(maxsize=None)
def _run(s, k):
    """One guarded call with every output."""
    return _call(_inputs(s, k), want_logits=True, canary=GUARD)


@pytest.mark.parametrize("s, k", CASES, ids=IDS)
def test_regression_dz_is_gy_bitwise(s, k):
    c, got = _inputs(s, k), _run(s, k)
    assert got["logits"].shape == c["gy"].shape
    assert np.array_equal(_bits(got["logits"][:, c["ncls"]:]), _bits(c["gy"][:, c["ncls"]:]))


@pytest.mark.parametrize("s, k", CASES, ids=IDS)
def test_class_dz_within_the_bound(s, k):
    c, got = _inputs(s, k), _run(s, k)
    ncls = c["ncls"]
    err = np.abs(got["logits"][:, :ncls].astype(np.float64) - hbr.dz64(c["y"], c["gy"], ncls)[:, :ncls])
    tol = hbr.dz_tolerance(c["y"], c["gy"], ncls)
    print("max error / bound", (err / tol).max())
    assert (err <= tol).all(), (err / tol).max()
    cls = got["logits"][:, :ncls]
    assert cls.any() and not cls[hbr.zero_class_region(cls.shape)].any()           # S = 0 and gy = 0 give dz = 0


@pytest.mark.parametrize("s, k", CASES, ids=IDS)
def test_contractions_are_the_chains_on_the_devices_dz_bitwise(s, k):
    c, got = _inputs(s, k), _run(s, k)
    assert np.array_equal(_bits(got["features"]), _bits(hbr.grad_features(c["w"], got["logits"])))
    dW, db = hbr.grad_weight_bias(c["x"], got["logits"], T)
    assert np.array_equal(_bits(got["weight"]), _bits(dW))
    assert np.array_equal(_bits(got["bias"]), _bits(db))


@pytest.mark.parametrize("s, k", CASES, ids=IDS)
def test_guards_are_intact(s, k):
    check_guards(_run(s, k)["guards"], GUARD, {"features", "weight", "bias", "logits", "scratch"})


@pytest.mark.parametrize("s, k", CASES, ids=IDS)
def test_optional_outputs_do_not_change_the_others(s, k):
    c, full = _inputs(s, k), _run(s, k)
    for off in ({"want_features": False}, {"want_weight": False, "want_bias": False}, {"want_weight": False},
                {"want_features": False, "want_weight": False, "want_bias": False}, {}):
        kw = dict({"want_logits": True}, **off) if off else {"want_logits": False}
        got = _call(c, canary=GUARD, **kw)
        names = {"features", "weight", "bias", "logits"} - {n[5:] for n, v in kw.items() if not v}
        assert set(got) == names | {"guards"}, kw
        for name in names:
            assert np.array_equal(_bits(got[name]), _bits(full[name])), (kw, name)
        check_guards(got["guards"], GUARD, names | {"scratch"}, where=kw)


@pytest.mark.parametrize("s, k", CASES, ids=IDS)
def test_two_runs_give_the_same_bytes(s, k):
    again, full = _call(_inputs(s, k), want_logits=True), _run(s, k)
    for name in ("features", "weight", "bias", "logits"):
        assert np.array_equal(_bits(again[name]), _bits(full[name])), name


@pytest.mark.parametrize("s, k", [(1, 0), (2, 0), (5, 0)], ids=["3x24x7x33", "2x512x16x40", "2x40x1x%d" % (2 * T + 37)])
def test_a_frame_alone_and_inside_a_batch(s, k):
    c, full = _inputs(s, k), _run(s, k)
    for f in range(SHAPES[s][0]):
        alone = _call(c, frames=slice(f, f + 1), want_logits=True, want_weight=False, want_bias=False)
        assert np.array_equal(_bits(alone["features"][0]), _bits(full["features"][f])), f
        assert np.array_equal(_bits(alone["logits"][0]), _bits(full["logits"][f])), f


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("s, k", SMALL + [(2, 0)], ids=SMALL_IDS + ["2x512x16x40-19+2"])
def test_half_features(s, k, dtype):
    """dW / db are bitwise the fp32 call on the widened features, dX is the fp32 call's dX rounded to nearest even
    (y and gy are the case's: the backward does not ask where y came from)."""
    torch, dev = _torch()
    c = _inputs(s, k)
    xh = torch.tensor(c["x"], device=dev).to(getattr(torch, dtype))
    half = _call(c, x=xh, want_logits=True, canary=GUARD)
    wide = _call(c, x=xh.float(), want_logits=True)
    assert half["features"].dtype.itemsize == 2
    for name in ("weight", "bias", "logits"):
        assert np.array_equal(_bits(half[name]), _bits(wide[name])), name
    rounded = _np(torch.tensor(wide["features"]).to(getattr(torch, dtype)))
    assert np.array_equal(_bits(half["features"]), _bits(rounded))
    check_guards(half["guards"], GUARD)


# ---- is_semantic_nll ----

def _targets(shape, ncls, seed):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, ncls, shape)
    t[rng.random(shape) < 0.2] = 255
    return t


@pytest.mark.parametrize("dtype", ["uint8", "int32"])
@pytest.mark.parametrize("s, k", SMALL + [(3, 0)], ids=SMALL_IDS + [IDS[3]])
def test_semantic_nll(s, k, dtype):
    torch, dev = _torch()
    c = _inputs(s, k)
    ncls, y = c["ncls"], c["y"]
    t = _targets((y.shape[0],) + y.shape[2:], ncls, seed=500 + s)
    want, V, bad, grad = hbr.nll64(y, t, ncls)
    tt = torch.tensor(t.astype(dtype), device=dev)
    loss, valid, nbad, g, guards = core.semantic_nll(torch.tensor(y, device=dev), tt, ncls, canary=GUARD)
    got = loss.cpu().numpy()[0]
    w32 = np.float32(want)
    assert got in (w32, np.nextafter(w32, np.float32(np.inf)), np.nextafter(w32, np.float32(-np.inf))), (got, want)
    assert int(valid.item()) == V and int(nbad.item()) == 0 == bad
    assert np.array_equal(_bits(g.cpu().numpy()), _bits(grad))
    check_guards(guards, GUARD, {"loss", "valid_count", "bad_count", "grad", "scratch"})
    # twice the same bytes
    again = core.semantic_nll(torch.tensor(y, device=dev), tt, ncls)
    assert np.array_equal(_bits(again[0].cpu().numpy()), _bits(loss.cpu().numpy()))


def test_semantic_nll_in_place_inside_a_wider_tensor():
    """cnn_out is read as it lies (all CH planes per frame), the gradient is written into the class planes of a gy
    tensor whose regression planes stay as they are."""
    torch, dev = _torch()
    c = _inputs(1, 1)                                            # 3 frames, 19 + 3 channels
    ncls, y = c["ncls"], c["y"]
    t = _targets((y.shape[0],) + y.shape[2:], ncls, seed=7)
    want, V, bad, grad = hbr.nll64(y, t, ncls)
    gy = torch.full(y.shape, 7.0, dtype=torch.float32, device=dev)
    yd = torch.tensor(y, device=dev)
    loss, valid, nbad, g = core.semantic_nll(yd[:, :ncls], torch.tensor(t.astype(np.uint8), device=dev), ncls, grad=gy)
    assert g.data_ptr() == gy.data_ptr() and int(valid.item()) == V
    h = gy.cpu().numpy()
    assert np.array_equal(_bits(h[:, :ncls]), _bits(grad)) and (h[:, ncls:] == 7.0).all()
    assert abs(float(loss.item()) - want) <= np.spacing(np.float32(want))


def test_semantic_nll_edge_cases():
    torch, dev = _torch()
    c = _inputs(1, 0)
    ncls, y = c["ncls"], c["y"]
    yd = torch.tensor(y, device=dev)
    shape = (y.shape[0],) + y.shape[2:]
    # no valid pixel: NaN, zero counts, a zero gradient
    loss, valid, nbad, g = core.semantic_nll(yd, torch.full(shape, 255, dtype=torch.uint8, device=dev), ncls)
    assert np.isnan(loss.item()) and valid.item() == 0 and nbad.item() == 0 and not g.cpu().numpy().any()
    # one frame ignored; bad targets (int32: negative and too large) are ignored and counted, check=True raises
    t = _targets(shape, ncls, seed=9)
    t[1] = 255
    t[0, 0, 0], t[2, 1, 1] = ncls, -1
    want, V, bad, grad = hbr.nll64(y, t, ncls)
    assert bad == 2
    td = torch.tensor(t.astype(np.int32), device=dev)
    loss, valid, nbad, g = core.semantic_nll(yd, td, ncls, check=False)
    assert valid.item() == V and nbad.item() == 2 and np.array_equal(_bits(g.cpu().numpy()), _bits(grad))
    assert abs(float(loss.item()) - want) <= np.spacing(np.float32(want))
    with pytest.raises(core.CoreError, match="2 targets"):
        core.semantic_nll(yd, td, ncls)


# ---- end to end through torch.autograd ----

def _module(c, dev):
    import torch
    CH, K = c["w"].shape
    head = training.SegmentationHead(K, c["ncls"], CH - c["ncls"]).to(dev)
    assert head.weight.shape == (CH, K, 1, 1) and head.bias.shape == (CH,) and not head.bias.any()
    bias = (np.random.default_rng(1).standard_normal(CH) * 0.1).astype(np.float32)
    head.load_state_dict({"weight": torch.tensor(c["w"]).reshape(CH, K, 1, 1), "bias": torch.tensor(bias)})
    return head, bias


def test_training_step_equals_the_direct_calls(monkeypatch):
    torch, dev = _torch()
    c = _inputs(1, 0)                                            # 3 x 24 x 7 x 33, 19 + 2
    ncls = c["ncls"]
    n, K, Hs, Ws = c["x"].shape
    head, bias = _module(c, dev)
    target = torch.tensor(_targets((n, Hs, Ws), ncls, seed=11).astype(np.uint8), device=dev)
    ids = np.random.default_rng(12).choice(np.array([0, 5, 26, 255, 1001, 1002, 26001], np.int32), (n, Hs, Ws))
    ids8 = torch.tensor(ids, device=dev)
    closs, rloss = training.SemanticNLLLoss(n_classes=ncls), training.OffsetLossSL()
    calls = []
    real = core.segmentation_head_backward
    monkeypatch.setattr(core, "segmentation_head_backward",
                        lambda *a, **kw: calls.append(kw) or real(*a, **kw))

    features = torch.tensor(c["x"], device=dev, requires_grad=True)
    out = head(features)
    loss = closs(out, target) + rloss(out[:, ncls:], ids8)
    loss.backward()
    assert len(calls) == 1 and calls[0]["want_features"] and calls[0]["want_weight"] and calls[0]["want_bias"]

    # the same step from the core calls
    y = core.segmentation_head(features.detach(), c["w"], bias, ncls, 8, want_segmentation=False)
    assert np.array_equal(_bits(out.detach().cpu().numpy()), _bits(y.cpu().numpy()))
    gy = torch.empty_like(y)
    l_cls = core.semantic_nll(y, target, ncls, grad=gy)[0]
    l5, _, g_reg = core.offset_loss(y[:, ncls:], ids8, None, weights=(1e-3, 1e-4, 0.0, 0.0))
    gy[:, ncls:] = g_reg
    assert np.array_equal(_bits(loss.detach().cpu().numpy()), _bits((l_cls[0] + l5[0]).cpu().numpy()))
    g = real(features.detach(), head.weight.detach(), y, gy, ncls)
    assert np.array_equal(_bits(features.grad.cpu().numpy()), _bits(g["features"].cpu().numpy()))
    assert np.array_equal(_bits(head.weight.grad.cpu().numpy().reshape(-1, K)), _bits(g["weight"].cpu().numpy()))
    assert np.array_equal(_bits(head.bias.grad.cpu().numpy()), _bits(g["bias"].cpu().numpy()))

    # frozen features: no dX is produced
    head.zero_grad()
    calls.clear()
    frozen = torch.tensor(c["x"], device=dev)
    out = head(frozen)
    (closs(out, target) + rloss(out[:, ncls:], ids8)).backward()
    assert len(calls) == 1 and not calls[0]["want_features"] and frozen.grad is None
    assert np.array_equal(_bits(head.weight.grad.cpu().numpy().reshape(-1, K)), _bits(g["weight"].cpu().numpy()))
    assert np.array_equal(_bits(head.bias.grad.cpu().numpy()), _bits(g["bias"].cpu().numpy()))


def test_training_step_within_the_bound_of_float64_autograd():
    """The module's gradients against torch's own autograd of Conv2d -> -log_softmax -> cat -> NLLLoss in float64 on
    the same inputs (the regression planes get a fixed linear loss), within hbr.autograd_bounds."""
    torch, dev = _torch()
    c = _inputs(1, 0)
    ncls = c["ncls"]
    n, K, Hs, Ws = c["x"].shape
    head, bias = _module(c, dev)
    t = _targets((n, Hs, Ws), ncls, seed=13)
    reg = (np.random.default_rng(14).standard_normal((n, c["w"].shape[0] - ncls, Hs, Ws)) / 64.0).astype(np.float32)
    features = torch.tensor(c["x"], device=dev, requires_grad=True)
    out = head(features)
    loss = training.SemanticNLLLoss(n_classes=ncls)(out, torch.tensor(t.astype(np.int32), device=dev)) + \
        (out[:, ncls:] * torch.tensor(reg, device=dev)).sum()
    loss.backward()
    loss64, dX64, dW64, db64, _ = hbr.torch_autograd64(c["x"], c["w"], bias, ncls, t, reg)
    y = out.detach().cpu().numpy()
    gy = np.concatenate((hbr.nll64(y, t, ncls)[3], reg), axis=1)
    z_mag = np.einsum("ck,nkhw->nchw", np.abs(c["w"].astype(np.float64)), np.abs(c["x"].astype(np.float64)))
    bx, bw, bb = hbr.autograd_bounds(c["x"], c["w"], z_mag, y, gy, hbr.dz(y, gy, ncls), ncls, T)
    assert (np.abs(features.grad.cpu().numpy().astype(np.float64) - dX64) <= bx).all()
    assert (np.abs(head.weight.grad.cpu().numpy().reshape(-1, K).astype(np.float64) - dW64) <= bw).all()
    assert (np.abs(head.bias.grad.cpu().numpy().astype(np.float64) - db64) <= bb).all()


def test_eval_mode_clamp_refuses_to_be_differentiated():
    torch, dev = _torch()
    c = _inputs(1, 1)                                            # 19 + 3: channel 19 is the disparity
    CH, K = c["w"].shape
    head = training.SegmentationHead(K, 19, 3, clamp=(19, 0.0, 128.0)).to(dev)
    x = torch.tensor(c["x"], device=dev)
    head.eval()
    with pytest.raises(core.CoreError, match="not differentiable"):
        head(x)
    with torch.no_grad():
        y = head(x)
    assert y.shape == c["y"].shape and float(y[:, 19].min()) >= 0.0
    head.train()
    assert head(x).requires_grad
