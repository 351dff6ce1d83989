"""The backward pass of conv + BatchNorm (+ residual) (+ ReLU) at stride 2 (f22) on the device against
tests/conv_stride_backward_reference.py, pinned as f21 is: the masked gradient gh bit for bit (with `out` from a real
core.conv_bn_stride call), then dX, dW, dscale and dshift on the device's own gh -- bit for bit on inputs whose
arithmetic is exact in every order, within the derived bounds on random inputs (each bound test prints max(err / tol);
the limit of 1 stands as derived).  Then: features_add, guards, the +0 lattice of the 1x1, every choice of optional
outputs, batch invariance, determinism, dY at an image stride, stride 1 against is_conv_bn_backward, and the training
modules against the inference classes, the hand-chained calls and float64 autograd of the reference's modules."""
import functools

import numpy as np
import pytest
import torch

import conv_backward_reference as cbr
import conv_bn_reference as cb
import conv_stride_backward_reference as csr
from guards import check_guards
from instance_stixels_amd import cnn, core, training

pytestmark = pytest.mark.gpu

DTYPES = sorted(csr.DTYPES)
CASES = [(s, k, dt) for s in range(len(csr.SHAPES)) for k in csr.KERNELS for dt in DTYPES]
IDS = ["%s-k%d-%s" % (csr.SHAPE_IDS[s], k, dt) for s, k, dt in CASES]
DX_CASES = [c for c in CASES if csr.SHAPES[c[0]][1] % 32 == 0]
DX_IDS = [i for c, i in zip(CASES, IDS) if csr.SHAPES[c[0]][1] % 32 == 0]
GUARD = 64
DEV = torch.device("cuda", 0)
NAMES = ("features", "weight", "scale", "shift", "pre")


def _inputs(s, kernel, kind):
    return csr.exact_inputs(s, kernel) if kind == "exact" else csr.random_inputs(s, kernel)


def _dev(a, td=None):
    t = torch.from_numpy(np.array(a)).to(DEV)
    return t if td is None else t.to(td)


def _cpu(g):
    return {k: v.cpu() for k, v in g.items() if k != "guards"}


def _guards_intact(g):
    check_guards(g["guards"], GUARD)


@functools.lru_cache(maxsize=None)
def _run(s, kernel, dtype, kind):
    """The forward by core.conv_bn_stride (with a residual and ReLU), then three guarded backward calls on the same
    device operands: every output with an fp32 dX; with features_add and an fp32 dX; with features_add and a half dX."""
    c, td = _inputs(s, kernel, kind), csr.DTYPES[dtype]
    cin = csr.SHAPES[s][1]
    x, res, add = _dev(c["x"], td), _dev(c["res"], td), _dev(c["add"], td)
    out = core.conv_bn_stride(x, core.conv_pack_weights(c["w"].copy(), td), c["scale"], c["shift"], kernel, 2, 1, residual=res)
    assert tuple(out.shape[2:]) == csr.out_extents(s)
    dy, w, sc = _dev(c["dy"]), _dev(c["w"]), _dev(c["scale"])
    dx = cin % 32 == 0
    full = core.conv_bn_stride_backward(x, w, sc, out, dy, kernel, 2, want_features=dx, want_pre=True,
                                        grad_features_dtype=torch.float32, canary=GUARD)
    _guards_intact(full)
    assert set(full) == {n for n in NAMES if dx or n != "features"} | {"guards"}
    r = dict(out=out.cpu(), full=_cpu(full))
    if dx:
        a32 = core.conv_bn_stride_backward(x, w, sc, out, dy, kernel, 2, want_weight=False, want_scale=False,
                                           want_shift=False, features_add=add, grad_features_dtype=torch.float32,
                                           canary=GUARD)
        a16 = core.conv_bn_stride_backward(x, w, sc, out, dy, kernel, 2, want_weight=False, want_scale=False,
                                           want_shift=False, features_add=add, canary=GUARD)
        h16 = core.conv_bn_stride_backward(x, w, sc, out, dy, kernel, 2, want_weight=False, want_scale=False,
                                           want_shift=False, canary=GUARD)
        _guards_intact(a32), _guards_intact(a16), _guards_intact(h16)
        assert a16["features"].dtype == h16["features"].dtype == td and a32["features"].dtype == torch.float32
        r.update(add32=a32["features"].cpu(), add16=a16["features"].cpu(), half=h16["features"].cpu())
    return r


@functools.lru_cache(maxsize=None)
def _reference(s, kernel, dtype, kind, with_add):
    """The reference on the device's own gh."""
    c, got = _inputs(s, kernel, kind), _run(s, kernel, dtype, kind)
    return csr.backward(c["x"], c["w"], c["scale"], got["full"]["pre"], kernel, dtype, add=c["add"] if with_add else None)


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("s, kernel, dtype", CASES, ids=IDS)
def test_masked_gradient_is_bitwise(s, kernel, dtype, kind):
    c, got = _inputs(s, kernel, kind), _run(s, kernel, dtype, kind)
    want = cbr.masked_gradient(c["dy"], got["out"], True, dtype)
    assert torch.equal(got["full"]["pre"].view(torch.int16), want.view(torch.int16))
    assert (got["out"] > 0).any() and (got["out"] == 0).any()                     # ReLU cuts some and not all


@pytest.mark.parametrize("s, kernel, dtype", CASES, ids=IDS)
def test_exact_inputs_give_the_float64_reference_bitwise(s, kernel, dtype):
    got, r = _run(s, kernel, dtype, "exact"), _reference(s, kernel, dtype, "exact", False)
    f, td = got["full"], csr.DTYPES[dtype]
    for name, ref in (("weight", "dw"), ("scale", "dscale"), ("shift", "dshift"), ("features", "dx")):
        if name not in f:
            assert name == "features" and csr.SHAPES[s][1] % 32
            continue
        bad = f[name].numpy().astype(np.float64) != r[ref].astype(np.float32).astype(np.float64)
        assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    assert np.array_equal(r["dw"].astype(np.float32).astype(np.float64), r["dw"])      # (dW itself is an fp32 value)
    assert (r["dw"] != 0).any() and (r["dshift"] != 0).any()
    if "add32" in got:
        ra = _reference(s, kernel, dtype, "exact", True)
        assert np.array_equal(got["add32"].numpy().astype(np.float64), ra["dx"])
        assert np.array_equal(ra["dx"].astype(np.float32).astype(np.float64), ra["dx"])
        # to the half: the one rounding of the exact value, with and without the add
        for key, ref in (("add16", ra["dx"]), ("half", r["dx"])):
            want = torch.from_numpy(ref).to(td)
            assert torch.equal(got[key].double(), want.double()), key


@pytest.mark.parametrize("s, kernel, dtype", CASES, ids=IDS)
def test_random_inputs_stay_within_the_bounds(s, kernel, dtype):
    """Measured on the MI355X: the table in DESIGN.md 10ab; the limits of 1 stand as derived."""
    got, r = _run(s, kernel, dtype, "random"), _reference(s, kernel, dtype, "random", False)
    f, worst = got["full"], {}
    for name, ref in (("features", "dx"), ("weight", "dw"), ("scale", "dscale"), ("shift", "dshift")):
        if name in f:
            worst[ref] = float((np.abs(f[name].numpy().astype(np.float64) - r[ref]) / r["tol_" + ref]).max())
    if "add32" in got:
        ra = _reference(s, kernel, dtype, "random", True)
        worst["dx+add"] = float((np.abs(got["add32"].numpy().astype(np.float64) - ra["dx"]) / ra["tol_dx"]).max())
    print("conv_bn_stride_backward %s k%d %s: max err / tol %s" % (csr.SHAPE_IDS[s], kernel, dtype,
                                                                  " ".join("%s %.5f" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("s, kernel, dtype", DX_CASES, ids=DX_IDS)
def test_half_dx_is_the_rne_conversion_of_the_fp32_dx(s, kernel, dtype, kind):
    """features_add is added in fp32 before the single final rounding; without it the half dX is the rounded fp32 one."""
    got, td = _run(s, kernel, dtype, kind), csr.DTYPES[dtype]
    assert torch.equal(got["add16"].view(torch.int16), got["add32"].to(td).view(torch.int16))
    assert torch.equal(got["half"].view(torch.int16), got["full"]["features"].to(td).view(torch.int16))
    assert not torch.equal(got["add32"], got["full"]["features"])              # (the add did something)


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("s, dtype", [(c[0], c[2]) for c in DX_CASES if c[1] == 1])
def test_a_1x1_writes_plus_zero_off_the_even_lattice(s, dtype, kind):
    """At kernel 1 only (even, even) elements get a sum: every other element is exactly +0, or the features_add value,
    in the fp32 and in the half output; and every element is written (the guarded buffers start as a non-zero pattern)."""
    c, got, td = _inputs(s, 1, kind), _run(s, 1, dtype, kind), csr.DTYPES[dtype]
    Hi, Wi = csr.SHAPES[s][3:]
    off = np.ones((Hi, Wi), bool)
    off[::2, ::2] = False
    assert (got["full"]["features"].view(torch.int32).numpy()[:, :, off] == 0).all()
    assert (got["half"].view(torch.int16).numpy()[:, :, off] == 0).all()
    add = torch.from_numpy(c["add"].copy()).to(td)
    assert np.array_equal(got["add16"].view(torch.int16).numpy()[:, :, off], add.view(torch.int16).numpy()[:, :, off])
    assert np.array_equal(got["add32"].numpy()[:, :, off], add.float().numpy()[:, :, off])
    for key in ("add32", "add16", "half"):
        assert torch.isfinite(got[key].float()).all(), key
    if Hi > 1 or Wi > 1:
        assert off.any()
    assert got["full"]["features"].numpy()[:, :, ::2, ::2].any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel", csr.KERNELS)
def test_dx_is_refused_at_layer2s_16_channels(kernel, dtype):
    s = len(csr.SHAPES) - 1
    c, td = csr.random_inputs(s, kernel), csr.DTYPES[dtype]
    assert csr.SHAPES[s][1] == 16
    x = _dev(c["x"], td)
    out = torch.ones(c["dy"].shape, dtype=td, device=DEV)
    with pytest.raises(core.CoreError, match="channels_in % 32"):
        core.conv_bn_stride_backward(x, _dev(c["w"]), c["scale"], out, out, kernel, 2)
    got = _run(s, kernel, dtype, "random")["full"]
    assert "features" not in got and all(torch.isfinite(got[n]).all() and got[n].any() for n in ("weight", "scale", "shift"))


SUBSETS = [(3, 3, "float16"), (4, 1, "bfloat16"), (6, 3, "bfloat16"), (5, 1, "float16"), (8, 3, "float16")]


@pytest.mark.parametrize("s, kernel, dtype", SUBSETS)
def test_every_choice_of_outputs_and_two_runs_give_the_same_bytes(s, kernel, dtype):
    c, td = csr.random_inputs(s, kernel), csr.DTYPES[dtype]
    first = _run(s, kernel, dtype, "random")
    x, out, dy, w, sc = _dev(c["x"], td), first["out"].to(DEV), _dev(c["dy"]), _dev(c["w"]), _dev(c["scale"])
    names = [n for n in NAMES if n in first["full"]]
    choices = [(n,) for n in names] + [("weight", "scale"), ("scale", "shift"), tuple(names)]
    if "features" in names:     # gh in the scratch (no "pre") beside the transposed pack, with and without the partials
        choices += [("features", "weight"), ("features", "shift")]
    for chosen in choices:
        want = {"want_" + n: n in chosen for n in NAMES}
        g = core.conv_bn_stride_backward(x, w, sc, out, dy, kernel, 2, grad_features_dtype=torch.float32, canary=GUARD, **want)
        _guards_intact(g)
        assert set(g) == set(chosen) | {"guards"}
        for n in chosen:
            a, b = g[n].cpu().contiguous(), first["full"][n].contiguous()
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (chosen, n)


@pytest.mark.parametrize("s, kernel, dtype", [(6, 3, "bfloat16"), (7, 1, "float16")])
def test_a_frame_alone_and_inside_a_batch(s, kernel, dtype):
    c, td = csr.random_inputs(s, kernel), csr.DTYPES[dtype]                    # three images
    got = _run(s, kernel, dtype, "random")
    x, out, dy = _dev(c["x"], td), got["out"].to(DEV), _dev(c["dy"])
    for f in (0, 1, 2):
        g = core.conv_bn_stride_backward(x[f:f + 1], _dev(c["w"]), c["scale"], out[f:f + 1], dy[f:f + 1], kernel, 2,
                                         want_weight=False, want_scale=False, want_shift=False, want_pre=True,
                                         grad_features_dtype=torch.float32)
        assert torch.equal(g["pre"].cpu().view(torch.int16), got["full"]["pre"][f:f + 1].view(torch.int16))
        assert torch.equal(g["features"].cpu().view(torch.int32), got["full"]["features"][f:f + 1].view(torch.int32))


@pytest.mark.parametrize("s, kernel, dtype", SUBSETS[:2])
def test_dy_is_read_in_place_at_an_image_stride(s, kernel, dtype):
    c, td = csr.random_inputs(s, kernel), csr.DTYPES[dtype]
    got = _run(s, kernel, dtype, "random")
    n, cin, cout = csr.SHAPES[s][:3]
    Ho, Wo = csr.out_extents(s)
    reps = max(n, 2) // n
    wide = torch.full((max(n, 2), cout + 3, Ho, Wo), float("nan"), device=DEV)
    x = _dev(np.concatenate([c["x"]] * reps), td)
    out = torch.cat([got["out"]] * reps).to(DEV)
    wide[:, :cout] = _dev(np.concatenate([c["dy"]] * reps))
    dy = wide[:, :cout]
    assert core._planes_in_place(dy, cout) and not dy.is_contiguous()
    a = core.conv_bn_stride_backward(x, _dev(c["w"]), c["scale"], out, dy, kernel, 2, want_pre=True)
    b = core.conv_bn_stride_backward(x, _dev(c["w"]), c["scale"], out, dy.contiguous(), kernel, 2, want_pre=True)
    for name in a:
        assert torch.equal(a[name].contiguous().view(torch.uint8), b[name].contiguous().view(torch.uint8)), name
    assert torch.isfinite(a["weight"]).all() and torch.isfinite(a["shift"]).all() and torch.isfinite(a["features"].float()).all()
    assert torch.equal(a["pre"][:n].cpu().view(torch.int16), got["full"]["pre"].view(torch.int16))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s, kernel", [(5, 3), (8, 1), (9, 3)])
def test_stride_1_gives_the_bytes_of_conv_bn_backward(s, kernel, dtype):
    """f21's shapes through the new entry point: the same launches, so the same bytes for every output."""
    c, td, d = cbr.random_inputs(s, kernel), cbr.DTYPES[dtype], cbr.dilation_of(s, kernel)
    x, res, add = _dev(c["x"], td), _dev(c["res"], td), _dev(c["add"], td)
    out = core.conv_bn(x, core.conv_pack_weights(c["w"].copy(), td), c["scale"], c["shift"], kernel, d, residual=res)
    dy, w, sc = _dev(c["dy"]), _dev(c["w"]), _dev(c["scale"])
    dx = cbr.SHAPES[s][1] % 32 == 0
    more = dict(want_features=dx, want_pre=True, features_add=add if dx else None, canary=GUARD)
    old = core.conv_bn_backward(x, w, sc, out, dy, kernel, d, **more)
    new = core.conv_bn_stride_backward(x, w, sc, out, dy, kernel, 1, d, **more)
    _guards_intact(old), _guards_intact(new)
    assert set(old) == set(new) and len(old) == (6 if dx else 5)
    for name in old:
        if name != "guards":
            assert torch.equal(old[name].contiguous().view(torch.uint8), new[name].contiguous().view(torch.uint8)), name


# ---- the training modules ----

def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and \
        torch.equal(a.detach().reshape(-1).view(torch.uint8), b.detach().reshape(-1).view(torch.uint8))


def _features(n, c, H, W, td, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, c, H, W, generator=g).abs()).to(DEV).to(td)


def _fold_grads(bn, dscale, dshift):
    """(dscale, dshift) sent on through the fold of a frozen BatchNorm by the ops the modules use: bn.weight's and
    bn.bias's gradients."""
    f = training._FrozenBatchNorm(bn).to(DEV)
    torch.autograd.backward(list(f.fold()), [dscale, dshift])
    return f.weight.grad, f.bias.grad


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cin", [16, 32])
def test_strided_conv_bn_relu_module_equals_the_direct_calls(cin, dtype):
    td = csr.DTYPES[dtype]
    conv = torch.nn.Conv2d(cin, 32, 3, stride=2, padding=1, bias=False)
    bn = cb.batchnorm(32, 5).eval()
    layer = training.StridedConvBnReLU(conv, bn).to(DEV)
    x = _features(2, cin, 9, 33, td, 1).requires_grad_(cin == 32)
    y = layer(x)
    assert tuple(y.shape) == (2, 32, 5, 17)
    assert _bits_equal(y, cnn.StridedConvBnRelu(conv, bn, dtype=td, device=DEV)(x.detach()))     # the inference class
    gy = _features(2, 32, 5, 17, td, 2) - 0.5
    y.backward(gy)
    scale, shift = (t.to(DEV) for t in cnn.fold_batchnorm(bn))
    g = core.conv_bn_stride_backward(x.detach(), layer.weight, scale, y.detach(), gy, 3, 2, want_features=cin == 32)
    assert _bits_equal(layer.weight.grad, g["weight"])
    if cin == 32:
        assert _bits_equal(x.grad, g["features"])
    gw, gb = _fold_grads(bn, g["scale"], g["shift"])
    assert _bits_equal(layer.bn.weight.grad, gw) and _bits_equal(layer.bn.bias.grad, gb) and _bits_equal(gb, g["shift"])
    if cin == 16:                                                  # dX at 16 channels is refused by the C ABI
        with pytest.raises(core.CoreError, match="channels_in % 32"):
            layer(x.detach().requires_grad_(True)).backward(gy)


def _block_by_hand(ref, block, x, y, gy, td, need_x=True):
    """The backward of a BasicBlock by hand: conv2's call, the downsample's, conv1's with the second path joined inside
    its launch.  Returns {parameter name: gradient} and the input's gradient."""
    stride, d1, d2 = int(ref.conv1.stride[0]), int(ref.conv1.dilation[0]), int(ref.conv2.dilation[0])
    fold = lambda bn: [t.to(DEV) for t in cnn.fold_batchnorm(bn)]
    f1, f2 = fold(ref.bn1), fold(ref.bn2)
    y1 = core.conv_bn_stride(x, core.conv_pack_weights(block.weight1.detach(), td), f1[0], f1[1], 3, stride, d1)
    residual, down = bool(ref.residual), ref.downsample if ref.residual else None
    g2 = core.conv_bn_backward(y1, block.weight2, f2[0], y, gy, 3, d2, want_pre=residual)
    grads, add = {}, None
    if down is not None:
        fd = fold(down[1])
        gd = core.conv_bn_stride_backward(x, block.weight_down, fd[0], None, g2["pre"], 1, stride, relu=False,
                                          want_features=need_x)
        add = gd.get("features")
        grads["weight_down"] = gd["weight"]
        grads["bn_down.weight"], grads["bn_down.bias"] = _fold_grads(down[1], gd["scale"], gd["shift"])
    elif residual:
        add = g2["pre"]
    g1 = core.conv_bn_stride_backward(x, block.weight1, f1[0], y1, g2["features"], 3, stride, d1, want_features=need_x,
                                      features_add=add if need_x else None)
    grads["weight1"], grads["weight2"] = g1["weight"], g2["weight"]
    grads["bn1.weight"], grads["bn1.bias"] = _fold_grads(ref.bn1, g1["scale"], g1["shift"])
    grads["bn2.weight"], grads["bn2.bias"] = _fold_grads(ref.bn2, g2["scale"], g2["shift"])
    return grads, g1.get("features")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cin, cout", [(32, 64), (64, 128)])
def test_strided_basic_block_module_equals_the_direct_calls(cin, cout, dtype):
    td = csr.DTYPES[dtype]
    ref = cb.Block(cin, cout, dilation=(1, 1), downsample=True, stride=2, seed=11).eval()
    block = training.StridedBasicBlock(ref).to(DEV)
    x = _features(2, cin, 9, 33, td, 3).requires_grad_(True)
    y = block(x)
    assert tuple(y.shape) == (2, cout, 5, 17)
    assert _bits_equal(y, cnn.StridedResidualBlock(ref, dtype=td, device=DEV)(x.detach()))
    gy = _features(2, cout, 5, 17, td, 4) - 0.5
    y.backward(gy)
    grads, gx = _block_by_hand(ref, block, x.detach(), y.detach(), gy, td)
    assert _bits_equal(x.grad, gx)
    named = dict(block.named_parameters())
    assert set(named) == set(grads) and len(grads) == 9
    for name, g in grads.items():
        assert _bits_equal(named[name].grad, g) and torch.isfinite(g).all() and g.any(), name


# ---- the whole modules against float64 autograd, on a family whose every intermediate is exact (as f21's) ----

def _exact_bn(channels, g):
    """eps = 2^-10, running_var = 1 - 2^-10 (their sum is 1 in every format): scale = weight in {-1, 1}, shift = bias -
    mean * weight, all integers."""
    bn = torch.nn.BatchNorm2d(channels, eps=2.0 ** -10).eval()
    with torch.no_grad():
        bn.weight.copy_(torch.randint(0, 2, (channels,), generator=g) * 2.0 - 1.0)
        bn.bias.copy_(torch.randint(-2, 3, (channels,), generator=g).float())
        bn.running_mean.copy_(torch.randint(-2, 3, (channels,), generator=g).float())
        bn.running_var.fill_(1.0 - 2.0 ** -10)
    return bn


def _sparse_weight(conv, g):
    """Weights in {-1, 0, 1}, one in eight non-zero: sums of a few dozen small integers."""
    with torch.no_grad():
        sign = torch.randint(0, 2, conv.weight.shape, generator=g) * 2.0 - 1.0
        conv.weight.copy_(sign * (torch.randint(0, 8, conv.weight.shape, generator=g) == 0))


def _grads_equal_bitwise(named_dev, named_ref):
    for name, got in named_dev.items():
        want = named_ref[name].to(got.dtype)                      # torch's conversion on the CPU: round to nearest even
        assert _bits_equal(got.cpu(), want) or torch.equal(got.cpu().double(), want.double()), name   # (-0 == +0)
        assert float(want.double().abs().max()) > 0, name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H, W", [(9, 33), (8, 34)])
def test_strided_basic_block_equals_float64_autograd_on_exact_inputs(H, W, dtype):
    """f21's family (x in {0, 1}, sparse weights in {-1, 0, 1}, BatchNorm with variance + eps = 1 and integer mean,
    weight and bias, dY integers in [-2, 2]) through conv_bn_reference.Block(..., stride=2): every intermediate is a
    small integer that both half dtypes hold, no ReLU mask can flip, and every gradient -- the input's, the three
    weights', every BatchNorm weight's and bias's -- must equal the float64 one, the input's after its one rounding."""
    td = csr.DTYPES[dtype]
    ref = cb.Block(32, 64, dilation=(1, 1), downsample=True, stride=2, seed=31)
    g = torch.Generator().manual_seed(31)
    ref.bn1, ref.bn2, ref.downsample[1] = _exact_bn(64, g), _exact_bn(64, g), _exact_bn(64, g)
    _sparse_weight(ref.conv1, g), _sparse_weight(ref.conv2, g), _sparse_weight(ref.downsample[0], g)
    ref = ref.eval()
    g = torch.Generator().manual_seed(5)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    x = torch.randint(0, 2, (2, 32, H, W), generator=g).float()
    dy = torch.randint(-2, 3, (2, 64, Ho, Wo), generator=g).float()
    block = training.StridedBasicBlock(ref).to(DEV)
    xd = x.to(DEV).to(td).requires_grad_(True)
    y = block(xd)
    y.backward(dy.to(DEV).to(td))
    r64 = ref.double()
    x64 = x.double().requires_grad_(True)
    y1 = torch.relu(r64.bn1(r64.conv1(x64)))
    y1.retain_grad()
    out = torch.relu(r64.bn2(r64.conv2(y1)) + r64.downsample(x64))
    out.backward(dy.double())
    for t in (y1.detach(), y1.grad):                              # the two intermediates that are stored as halves
        assert torch.equal(t.to(td).double(), t)
    assert torch.equal(y.detach().cpu().double(), out.detach().to(td).double())
    assert (y1.detach() > 0).any() and (y1.detach() == 0).any() and (out.detach() == 0).any()
    dev = {"x": xd.grad, "weight1": block.weight1.grad, "weight2": block.weight2.grad, "weight_down": block.weight_down.grad,
           "bn1.weight": block.bn1.weight.grad, "bn1.bias": block.bn1.bias.grad, "bn2.weight": block.bn2.weight.grad,
           "bn2.bias": block.bn2.bias.grad, "bn_down.weight": block.bn_down.weight.grad, "bn_down.bias": block.bn_down.bias.grad}
    want = {"x": x64.grad, "weight1": r64.conv1.weight.grad, "weight2": r64.conv2.weight.grad,
            "weight_down": r64.downsample[0].weight.grad, "bn1.weight": r64.bn1.weight.grad, "bn1.bias": r64.bn1.bias.grad,
            "bn2.weight": r64.bn2.weight.grad, "bn2.bias": r64.bn2.bias.grad,
            "bn_down.weight": r64.downsample[1].weight.grad, "bn_down.bias": r64.downsample[1].bias.grad}
    assert len(dev) == len(list(block.parameters())) + 1
    _grads_equal_bitwise(dev, want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cin, H, W", [(32, 9, 33), (16, 8, 34)])
def test_strided_conv_bn_relu_module_equals_float64_autograd_on_exact_inputs(cin, H, W, dtype):
    td = csr.DTYPES[dtype]
    g = torch.Generator().manual_seed(8)
    conv = torch.nn.Conv2d(cin, 64, 3, stride=2, padding=1, bias=False)
    _sparse_weight(conv, g)
    bn = _exact_bn(64, g)
    x = torch.randint(0, 2, (2, cin, H, W), generator=g).float()
    dy = torch.randint(-2, 3, (2, 64, (H + 1) // 2, (W + 1) // 2), generator=g).float()
    layer = training.StridedConvBnReLU(conv, bn).to(DEV)
    xd = x.to(DEV).to(td).requires_grad_(cin == 32)
    layer(xd).backward(dy.to(DEV).to(td))
    conv64, bn64 = conv.double(), bn.double()
    x64 = x.double().requires_grad_(True)
    torch.relu(bn64(conv64(x64))).backward(dy.double())
    dev = {"weight": layer.weight.grad, "bn.weight": layer.bn.weight.grad, "bn.bias": layer.bn.bias.grad}
    if cin == 32:
        dev["x"] = xd.grad
    _grads_equal_bitwise(dev, {"x": x64.grad, "weight": conv64.weight.grad, "bn.weight": bn64.weight.grad,
                               "bn.bias": bn64.bias.grad})


def _reduced_layers(width=32):
    seq = lambda ci, co, s, d, seed: torch.nn.Sequential(
        torch.nn.Conv2d(ci, co, 3, stride=s, padding=d, dilation=d, bias=False), cb.batchnorm(co, seed), torch.nn.ReLU())
    blocks = lambda stride, d, down, seed: torch.nn.Sequential(
        cb.Block(width, width, dilation=d, downsample=down, stride=stride, seed=seed),
        cb.Block(width, width, dilation=d, seed=seed + 5))
    torch.manual_seed(3)
    return [m.eval() for m in (seq(16, width, 2, 1, 41), blocks(2, (1, 1), True, 50), blocks(2, (1, 1), True, 60),
                               blocks(1, (2, 2), True, 70), blocks(1, (4, 4), False, 80), seq(width, width, 1, 2, 42),
                               seq(width, width, 1, 1, 43))]


@pytest.mark.parametrize("dtype", DTYPES)
def test_drn_layers_equal_the_hand_chained_calls(dtype):
    """layer2 .. layer8 with every width reduced to 32 on a 2 x 16 x 19 x 35 input, followed by SegmentationHead and
    SemanticNLLLoss: the forward is the inference classes' (cnn), and every parameter gradient equals the core calls
    chained by hand from the gradient that reaches layer8's output, bit for bit; two steps give the same bytes."""
    td = csr.DTYPES[dtype]
    layers = _reduced_layers()
    net = training.DrnLayers(*layers).to(DEV)
    torch.manual_seed(11)
    head = training.SegmentationHead(32, 5, 2).to(DEV)
    nll = training.SemanticNLLLoss(n_classes=5)
    x = _features(2, 16, 19, 35, td, 9)
    g = torch.Generator().manual_seed(4)
    target = torch.randint(0, 5, (2, 3, 5), generator=g).to(torch.uint8)
    target[0, :1] = 255

    def step():
        net.zero_grad(), head.zero_grad()
        out = net(x)
        out.retain_grad()
        nll(head(out), target.to(DEV)).backward()
        return out.detach(), out.grad.clone(), {n: p.grad.clone() for n, p in net.named_parameters()}

    out, gout, grads = step()
    assert tuple(out.shape) == (2, 32, 3, 5) and out.dtype == td
    # the forward: the inference classes, launch for launch
    refs = [layers[0]] + [b for layer in layers[1:5] for b in layer] + layers[5:]
    f, saved = x, []
    for ref in refs:
        saved.append(f)
        if isinstance(ref, torch.nn.Sequential):
            f = cnn.StridedConvBnRelu(ref[0], ref[1], dtype=td, device=DEV)(f)
        else:
            f = cnn.StridedResidualBlock(ref, dtype=td, device=DEV)(f)
    saved.append(f)
    assert _bits_equal(out, f)
    # the backward by hand, from layer8 down to layer2
    gy, seen = gout, 0
    for i in reversed(range(len(refs))):
        ref, mod, xin, y = refs[i], net.layers[i], saved[i], saved[i + 1]
        prefix = "layers.%d." % i
        if isinstance(ref, torch.nn.Sequential):
            conv, bn = ref[0], ref[1]
            scale = cnn.fold_batchnorm(bn)[0].to(DEV)
            gg = core.conv_bn_stride_backward(xin, mod.weight, scale, y, gy, 3, int(conv.stride[0]), int(conv.dilation[0]),
                                              want_features=i > 0)
            want = {"weight": gg["weight"]}
            want["bn.weight"], want["bn.bias"] = _fold_grads(bn, gg["scale"], gg["shift"])
            gy = gg.get("features")
        else:
            want, gy = _block_by_hand(ref, mod, xin, y, gy, td)
        for name, gw in want.items():
            assert _bits_equal(grads[prefix + name], gw), prefix + name
            assert torch.isfinite(gw).all() and gw.any(), prefix + name
            seen += 1
    assert seen == len(grads) == 3 + 3 * 9 + 5 * 6 + 2 * 3 and gy is None
    out2, gout2, grads2 = step()
    assert _bits_equal(out, out2) and _bits_equal(gout, gout2) and all(_bits_equal(grads[n], grads2[n]) for n in grads)
    with pytest.raises(core.CoreError, match="requires grad: the stem is frozen"):
        net(x.clone().requires_grad_(True))
