"""f12 on the MI355X: is_offset_loss (is_k_offset_loss.hip), core.offset_loss and training.OffsetLossSL /
DisparityOffsetLossSL against the float64 definition: the reference's own classes run in float64
(tests/golden/reference_python_losses) and the numpy restatement pinned on them (tests/offset_loss_reference.py).
Canary bytes around every output of the C ABI, the scratch included, must survive.

The bound is 2 float32 ulp on every term, loss and gradient element, NaN where the definition has NaN, exact zeros
exact.  It is derived, not measured: binary64 arithmetic rounded once gives 0.5 ulp; the fixture keeps every sign
argument out of (0, 1e-4) and the shapes keep cancellation out, so the error of another binary64 summation order is
orders below a float32 ulp; the rest is room for a rounding boundary."""
import numpy as np
import pytest

import offset_loss_reference as lr
from instance_stixels_amd import core
from test_offset_loss import case, fixture
from test_render_gpu import Out, _dev, _torch

pytestmark = pytest.mark.gpu
FILL = 0x5C   # the garbage Out() starts with
ULPS = 2.0
CH = 22       # the channels of the wider tensor a prediction is sliced out of


def _shifted(a, offset):
    """A device copy of `a` that starts `offset` bytes into a larger buffer."""
    torch, dev = _torch()
    b = np.ascontiguousarray(a).view(np.uint8).ravel()
    raw = torch.zeros(b.size + 64, dtype=torch.uint8, device=dev)
    raw[offset:offset + b.size] = _dev(b)
    return raw, raw.data_ptr() + offset


def _c_abi(pred, ids, d8=None, weights=(1e-3, 1e-4, 1e-3, 1e-4), abs_variance=False, capacity=0, want_terms=True,
           want_grad=True, sliced=False, odd=False):
    """is_offset_loss on host arrays with canaries around every output and the scratch.  sliced: prediction and
    gradient are the last channels of [n][CH][Hs][Ws] tensors.  odd: every input starts one element off.
    Returns dict(rc, loss, terms, grad, count, rest) as numpy."""
    torch, dev = _torch()
    pred = np.ascontiguousarray(pred, np.float32)
    n, planes, Hs, Ws = pred.shape
    cells = Hs * Ws
    stride = planes * cells
    if sliced:
        wide = np.random.default_rng(1).normal(0, 9, (n, CH, Hs, Ws)).astype(np.float32)
        wide[:, CH - planes:] = pred
        keep_p, p_pred = _shifted(wide, 4 if odd else 0)
        p_pred += (CH - planes) * cells * 4
        stride = CH * cells
        g = Out((n, CH, Hs, Ws), np.float32) if want_grad else None
    else:
        keep_p, p_pred = _shifted(pred, 4 if odd else 0)
        g = Out((n, planes, Hs, Ws), np.float32) if want_grad else None
    keep_i, p_ids = _shifted(np.asarray(ids, np.int32), 4 if odd else 0)
    keep_d, p_d8 = _shifted(np.asarray(d8, np.uint16), 2 if odd else 0) if planes == 3 else (None, None)
    loss, cnt = Out((5,), np.float32), Out((n,), np.int32)
    t = Out((n, 4), np.float32) if want_terms else None
    nbytes = core.offset_loss_scratch_bytes(n, planes, Hs, Ws, capacity)
    assert nbytes > 0
    scratch = Out((nbytes,), np.uint8, offset=0)
    assert scratch.ptr % 16 == 0
    torch.cuda.synchronize()
    rc = core.offset_loss_ptr(
        d_prediction=p_pred, prediction_image_stride=stride, d_ids8=p_ids, d_disparity8_u16=p_d8, n_images=n,
        planes=planes, rows8=Hs, cols8=Ws, w_offset_mean=weights[0], w_offset_variance=weights[1],
        w_disparity_mean=weights[2], w_disparity_variance=weights[3], abs_variance=int(abs_variance),
        d_loss=loss.ptr, d_terms=t.ptr if t else None,
        d_grad=(g.ptr + ((CH - planes) * cells * 4 if sliced else 0)) if g else None,
        grad_image_stride=stride if g else 0, capacity=capacity, d_scratch=scratch.ptr, scratch_bytes=nbytes,
        d_key_count=cnt.ptr)
    torch.cuda.synchronize()
    scratch.get()
    grad = rest = None
    if g:
        grad = g.get()
        if sliced:
            grad, rest = grad[:, CH - planes:], grad[:, :CH - planes]
    return dict(rc=rc, loss=loss.get(), terms=t.get() if t else None, grad=grad, count=cnt.get(), rest=rest)


def _within(got, want64, what):
    d = lr.ulp_distance(got, want64)
    worst = float(np.max(d)) if d.size else 0.0
    print(f"{what}: max {worst:.3f} ulp")
    assert worst <= ULPS, f"{what}: {worst} ulp at {np.unravel_index(np.argmax(d), d.shape)}"
    return worst


def _check(got, want, what=""):
    """got of _c_abi against (loss5, terms, grad) of the definition."""
    assert got["rc"] == 0, core.lib().is_last_error()
    _within(got["loss"], want[0], f"{what} loss")
    if got["terms"] is not None:
        _within(got["terms"], want[1], f"{what} terms")
    if got["grad"] is not None:
        _within(got["grad"], want[2], f"{what} gradient")
        assert np.isfinite(got["grad"]).all()


def _scene(n, Hs, Ws, seed, keys=12):
    """ids with blobs over stuff and non-contributing labels, q with holes, predictions."""
    rng = np.random.default_rng(seed)
    pool = np.array([7, 8, 10, 11, 21, 255, 1000, -4], np.int32)
    ids = pool[rng.integers(0, pool.size, (n, Hs // 4 + 1, Ws // 4 + 1))].repeat(4, 1).repeat(4, 2)[:, :Hs, :Ws].copy()
    q = rng.integers(0, 3, ids.shape) * 31
    for f in range(n):
        for k in range(keys):
            h, w = int(rng.integers(1, max(2, Hs // 2))), int(rng.integers(1, max(2, Ws // 2)))
            y0, x0 = int(rng.integers(0, Hs - h + 1)), int(rng.integers(0, Ws - w + 1))
            ids[f, y0:y0 + h, x0:x0 + w] = 24001 + 500 * (k % 5) + k
            q[f, y0:y0 + h, x0:x0 + w] = (int(rng.integers(1, 250)) + np.arange(h)[:, None] % 4) % 256
    q[rng.random(q.shape) < 0.15] = 0
    pred = np.stack([rng.normal(40, 25, ids.shape), rng.normal(0, 3, ids.shape), rng.normal(0, 4, ids.shape)], 1)
    d8 = (q * 256 + rng.integers(0, 256, q.shape)).astype(np.uint16)
    return pred.astype(np.float32), ids.astype(np.int32), d8


def _guarded(pred, ids, d8, weights):
    """Moves the predictions of a generated scene until no sign argument of the definition lies in (0, 1e-4): the rule
    the fixture's generator enforces, for the scenes made here (the abs form has every sign argument of the other)."""
    pred = pred.copy()
    for _ in range(20):
        bad = False
        for f in range(pred.shape[0]):
            args = {}
            lr.frame(pred[f], ids[f], d8[f] if d8 is not None else None, weights, True, sign_args=args)
            v = np.abs(np.concatenate([np.asarray(x, np.float64) for x in args.values()]))
            if ((v > 0) & (v < 1e-4)).any():
                bad = True
                pred[f] += np.float32(0.0078125)
        if not bad:
            return pred
    raise AssertionError("no guarded scene")


@pytest.fixture(scope="module")
def general3():
    """Three frames of 24 x 50 cells: the fixture's general frame, upside down, and rolled by (5, 13); their
    definition in float64 for both abs_variance settings."""
    z, _, weights = fixture()
    pred, ids, d8 = case(z, "general")
    p = np.stack([pred, pred[:, ::-1], np.roll(pred, (5, 13), (1, 2))])
    i = np.stack([ids, ids[::-1], np.roll(ids, (5, 13), (0, 1))])
    d = np.stack([d8, d8[::-1], np.roll(d8, (5, 13), (0, 1))])
    p = _guarded(p, i, d, weights)
    want = {a: lr.batch(p, i, d, weights, bool(a)) for a in (0, 1)}
    want2 = lr.batch(p[:, 1:], i, None, weights, False)
    return dict(pred=p, ids=i, d8=d, weights=weights, want=want, want2=want2)


@pytest.mark.parametrize("name", ["general", "no_keys", "no_stuff", "many_keys", "tiny"])
def test_c_abi_on_the_fixture_frames_against_the_reference_in_float64(name):
    """Every frame of the reference's own float64 run: 3 planes with both abs_variance settings, 2 planes against
    OffsetLossSL.  24 x 50 (waves straddle row ends, five workgroups, keys across them), 16 x 32 with 70 keys and
    with none, a frame without stuff (nan terms, a finite gradient), 2 x 3."""
    z, _, weights = fixture()
    pred, ids, d8 = case(z, name)
    worst_device = worst_float32 = 0.0
    for a in (0, 1):
        ref = f"{name}_d_D{a}"
        want = (np.concatenate([[z[f"{ref}_loss"]], z[f"{ref}_five"][1:]]), z[f"{ref}_five"][None, 1:], z[f"{ref}_grad"][None])
        got = _c_abi(pred[None], ids[None], d8[None], weights, a)
        _check(got, want, f"{name} abs_variance={a}")
        assert got["count"].tolist() == lr.key_counts(ids[None]).tolist()
        if name == "no_stuff":
            assert np.isnan(got["terms"][0, [0, 2]]).all() and np.isfinite(got["terms"][0, [1, 3]]).all()
        for key, mine in (("five", np.concatenate([got["loss"][:1], got["terms"][0]])), ("grad", got["grad"][0])):
            want64 = z[f"{ref}_{key}"]
            worst_device = max(worst_device, float(np.nanmax(lr.ulp_distance(mine, want64))))
            with np.errstate(invalid="ignore"):
                worst_float32 = max(worst_float32, float(np.nanmax(lr.ulp_distance(z[f"{name}_s_D{a}_{key}"], want64))))
    print(f"{name}: device {worst_device:.3f} ulp, the reference's float32 run {worst_float32:.3f} ulp")
    got = _c_abi(pred[None, 1:], ids[None], None, weights, 0)
    assert got["rc"] == 0
    _within(got["loss"][0], z[f"{name}_d_O0_loss"], "OffsetLossSL loss")
    _within(got["grad"][0], z[f"{name}_d_O0_grad"], "OffsetLossSL gradient")
    _within(got["terms"][0, :2], z[f"{name}_d_D0_five"][1:3], "OffsetLossSL terms")
    assert (got["terms"][0, 2:] == 0).all() and (got["loss"][3:] == 0).all()
    _check(_c_abi(pred[None, 1:], ids[None], None, weights, 1), lr.batch(pred[None, 1:], ids[None], None, weights, True),
           "2 planes, abs form")


@pytest.mark.parametrize("abs_variance", [0, 1])
def test_batch_variants_slices_odd_offsets_and_optional_outputs(general3, abs_variance):
    s = general3
    want = s["want"][abs_variance]
    plain = _c_abi(s["pred"], s["ids"], s["d8"], s["weights"], abs_variance)
    _check(plain, want, "batch")
    wide = _c_abi(s["pred"], s["ids"], s["d8"], s["weights"], abs_variance, sliced=True)
    assert (wide["rest"].view(np.uint8) == FILL).all(), "the other channels of the gradient tensor were written"
    odd = _c_abi(s["pred"], s["ids"], s["d8"], s["weights"], abs_variance, sliced=True, odd=True)
    for other in (wide, odd):
        for k in ("loss", "terms", "grad", "count"):
            assert other[k].tobytes() == plain[k].tobytes(), k
    bare = _c_abi(s["pred"], s["ids"], s["d8"], s["weights"], abs_variance, want_terms=False, want_grad=False)
    assert bare["rc"] == 0 and bare["loss"].tobytes() == plain["loss"].tobytes()
    if abs_variance == 0:
        got2 = _c_abi(s["pred"][:, 1:], s["ids"], None, s["weights"], 0, sliced=True, odd=True)
        _check(got2, s["want2"], "2 planes sliced")
        assert (got2["rest"].view(np.uint8) == FILL).all()


@pytest.mark.parametrize("zero", [0, 1, 2, 3])
def test_a_zero_weight_removes_its_gradient_lines_and_keeps_the_term(general3, zero):
    s = general3
    w = list(s["weights"])
    w[zero] = 0.0
    for a in (0, 1):
        got = _c_abi(s["pred"], s["ids"], s["d8"], w, a)
        _check(got, lr.batch(s["pred"], s["ids"], s["d8"], w, bool(a)), f"weight {zero} zero, abs_variance={a}")
        _within(got["terms"], s["want"][a][1], "the terms do not depend on the weights")
    # without stuff the nan term must not reach the gradient through a zero weight
    z, _, weights = fixture()
    pred, ids, d8 = case(z, "no_stuff")
    w = list(weights)
    w[zero] = 0.0
    _check(_c_abi(pred[None], ids[None], d8[None], w, 0), lr.batch(pred[None], ids[None], d8[None], w, False), "no stuff")


def test_more_than_64_chunks_per_frame_and_many_partitions():
    """72 x 64 cells = 72 chunks: two chunks per partition (the only other path of the partition), two frames."""
    w = (2.0 ** -10, 2.0 ** -13, 2.0 ** -9, 2.0 ** -12)
    pred, ids, d8 = _scene(2, 72, 64, seed=3)
    p = _guarded(pred, ids, d8, w)
    for a in (0, 1):
        _check(_c_abi(p, ids, d8, w, a), lr.batch(p, ids, d8, w, bool(a)), f"72x64 abs_variance={a}")


def test_capacity_exactly_enough_and_one_short():
    """The frame with 70 keys: capacity 70 gives the result; capacity 69 is the overflow contract: nan loss and terms
    for the batch, the gradient not written, the true counts."""
    z, _, weights = fixture()
    pred, ids, d8 = case(z, "many_keys")
    keys = int(lr.key_counts(ids[None])[0])
    assert keys >= 65
    _, ids0, _ = case(z, "no_keys")
    p2, i2, d2 = np.stack([pred, pred]), np.stack([ids0, ids]), np.stack([d8, d8])
    want = lr.batch(p2, i2, d2, weights, False)
    exact = _c_abi(p2, i2, d2, weights, 0, capacity=keys)
    _check(exact, want, "keys == capacity")
    assert exact["count"].tolist() == [0, keys]
    default = _c_abi(p2, i2, d2, weights, 0)
    for k in ("loss", "terms", "grad"):
        assert default[k].tobytes() == exact[k].tobytes(), k
    for planes in (3, 2):
        short = _c_abi(p2[:, 3 - planes:], i2, d2 if planes == 3 else None, weights, 0, capacity=keys - 1)
        assert short["rc"] == 0 and short["count"].tolist() == [0, keys]
        assert np.isnan(short["loss"]).all() and np.isnan(short["terms"]).all()
        assert (short["grad"].view(np.uint8) == FILL).all(), "the gradient was written on overflow"
    torch, dev = _torch()
    loss5, terms, grad, count = core.offset_loss(_dev(p2), _dev(i2), _dev(d2), weights=weights, capacity=16,
                                                 return_key_count=True)
    assert count.cpu().numpy().tolist() == [0, keys]
    for k, got in (("loss", loss5), ("terms", terms), ("grad", grad)):
        assert got.cpu().numpy().tobytes() == exact[k].tobytes(), k
    loss5, _, _ = core.offset_loss(_dev(p2), _dev(i2), _dev(d2), weights=weights, capacity=16, check=False)
    assert np.isnan(loss5.cpu().numpy()).all()


def test_same_bytes_on_every_run_under_permutation_and_alone(general3):
    s = general3
    for a in (0, 1):
        first = _c_abi(s["pred"], s["ids"], s["d8"], s["weights"], a)
        again = _c_abi(s["pred"], s["ids"], s["d8"], s["weights"], a)
        for k in ("loss", "terms", "grad", "count"):
            assert first[k].tobytes() == again[k].tobytes(), k
        perm = [2, 0, 1]
        moved = _c_abi(s["pred"][perm], s["ids"][perm], s["d8"][perm], s["weights"], a)
        for k in ("terms", "grad", "count"):
            assert moved[k].tobytes() == first[k][perm].tobytes(), k
        for f in range(3):
            alone = _c_abi(s["pred"][f:f + 1], s["ids"][f:f + 1], s["d8"][f:f + 1], s["weights"], a)
            for k in ("terms", "grad", "count"):
                assert alone[k].tobytes() == first[k][f:f + 1].tobytes(), (k, f)


def test_a_nan_prediction_stays_in_its_frame(general3):
    s = general3
    clean = _c_abi(s["pred"], s["ids"], s["d8"], s["weights"], 0)
    q = s["d8"][1] >> 8
    key = next(k for k in np.unique(s["ids"][1][s["ids"][1] > 1000]) if (q[s["ids"][1] == k] != 0).any())
    ys, xs = np.nonzero(s["ids"][1] == key)                                    # a key with a median
    for plane in (0, 1):
        p = s["pred"].copy()
        p[1, plane, ys[0], xs[0]] = np.nan
        got = _c_abi(p, s["ids"], s["d8"], s["weights"], 0)
        assert got["rc"] == 0
        hit = [2, 3] if plane == 0 else [0, 1]
        assert not np.isfinite(got["terms"][1, hit]).any() and not np.isfinite(got["loss"][0])
        for f in (0, 2):
            assert got["terms"][f].tobytes() == clean["terms"][f].tobytes()
            assert got["grad"][f].tobytes() == clean["grad"][f].tobytes()


def test_training_classes_backward_separate_and_overflow_recovery(general3):
    """pred = a * w with a = 2 and the leaf w = prediction / 2 (both products exact): w.grad is twice the gradient, and
    is compared with the torch loop of the reference's structure run on the device in float64 with autograd."""
    torch, dev = _torch()
    from instance_stixels_amd import training
    s = general3
    weights = s["weights"]
    kw = dict(offset_mean_weight=weights[0], offset_variance_weight=weights[1], disparity_mean_weight=weights[2],
              disparity_variance_weight=weights[3])
    pred, ids, d8 = s["pred"][:2], s["ids"][:2], s["d8"][:2]
    q = _dev((d8.astype(np.int64) >> 8).astype(np.float32))                    # the reference's tensor of integral q
    gt = _dev(ids.astype(np.int64))[:, None]                                   # [n][1][Hs][Ws] int64
    for a in (False, True):
        w64 = (_dev(pred).double() / 2).requires_grad_(True)
        loss64, sums64 = lr.torch_loop_loss(2.0 * w64, gt[:, 0], q.double(), weights, a)
        loss64.backward()
        w = (_dev(pred) / 2).requires_grad_(True)
        fn = training.DisparityOffsetLossSL(abs_variance=a, **kw)
        loss = fn(2.0 * w, gt, q)
        assert loss.dim() == 0 and loss.requires_grad
        loss.backward()
        _within(loss.detach().cpu().numpy(), loss64.item(), "training loss")
        _within(w.grad.cpu().numpy(), w64.grad.cpu().numpy(), "w.grad")
        five = fn(2.0 * w, gt, _dev(d8), separate=True)                         # raw uint16 too
        assert tuple(five.shape) == (5,) and not five.requires_grad
        _within(five.cpu().numpy(), [loss64.item()] + [float(v.detach()) for v in sums64], "separate")
    # OffsetLossSL on the last two channels of a wider tensor, ids [n][Hs][Ws] int32
    wide = torch.zeros((2, CH, 24, 50), device=dev)
    wide[:, CH - 2:] = _dev(pred[:, 1:])
    wide.requires_grad_(True)
    loss = training.OffsetLossSL(abs_variance=True, **kw)(wide[:, -2:], _dev(ids))
    loss.backward()
    want2 = lr.batch(pred[:, 1:], ids, None, weights)                          # (abs_variance is swallowed)
    _within(loss.detach().cpu().numpy(), want2[0][0], "OffsetLossSL")
    _within(wide.grad[:, CH - 2:].cpu().numpy(), want2[2], "OffsetLossSL gradient")
    assert (wide.grad[:, :CH - 2] == 0).all().item()
    # more keys than the capacity: check=True repeats with the reported count
    z, _, _ = fixture()
    p, i, d = case(z, "many_keys")
    fn = training.DisparityOffsetLossSL(capacity=16, check=True, **kw)
    t = _dev(p[None]).requires_grad_(True)
    loss = fn(t, _dev(i[None]), _dev(d[None]))
    loss.backward()
    want = lr.batch(p[None], i[None], d[None], weights, False)
    _within(loss.detach().cpu().numpy(), want[0][0], "recovered loss")
    _within(t.grad.cpu().numpy(), want[2], "recovered gradient")
