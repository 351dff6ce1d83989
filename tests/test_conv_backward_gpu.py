"""The backward pass of conv + BatchNorm (+ residual) (+ ReLU) (f21) on the device against
tests/conv_backward_reference.py, pinned in two stages as f13 / f14 are: the masked gradient gh bit for bit (with `out`
from a real core.conv_bn call), then dX, dW, dscale and dshift on the device's own gh -- bit for bit on inputs whose
arithmetic is exact in every order, within the derived bounds on random inputs (each bound test prints max(err / tol);
the limit of 1 stands as derived).  Then: features_add, guards, every choice of optional outputs, batch invariance,
determinism, dY at an image stride, and the training modules against the direct calls and, on a family whose every
intermediate is exact, against float64 autograd of the reference's modules."""
import functools

import numpy as np
import pytest
import torch

import conv_backward_reference as cbr
import conv_bn_reference as cb
from guards import check_guards
from instance_stixels_amd import cnn, core, training

pytestmark = pytest.mark.gpu

DTYPES = sorted(cbr.DTYPES)
CASES = [(s, k, dt) for s in range(len(cbr.SHAPES)) for k in cbr.KERNELS for dt in DTYPES]
IDS = ["%s-k%d-%s" % (cbr.SHAPE_IDS[s], k, dt) for s, k, dt in CASES]
GUARD = 64
DEV = torch.device("cuda", 0)
NAMES = ("features", "weight", "scale", "shift", "pre")


def _inputs(s, kernel, kind):
    return cbr.exact_inputs(s, kernel) if kind == "exact" else cbr.random_inputs(s, kernel)


def _dev(a, td=None):
    t = torch.from_numpy(np.array(a)).to(DEV)
    return t if td is None else t.to(td)


def _cpu(g):
    return {k: v.cpu() for k, v in g.items() if k != "guards"}


def _guards_intact(g):
    check_guards(g["guards"], GUARD)


@functools.lru_cache(maxsize=None)
def _run(s, kernel, dtype, kind):
    """The forward by core.conv_bn (with a residual and ReLU), then three guarded backward calls on the same device
    operands: every output with an fp32 dX; with features_add and an fp32 dX; with features_add and a half dX."""
    c, td, d = _inputs(s, kernel, kind), cbr.DTYPES[dtype], cbr.dilation_of(s, kernel)
    cin = cbr.SHAPES[s][1]
    x, res, add = _dev(c["x"], td), _dev(c["res"], td), _dev(c["add"], td)
    out = core.conv_bn(x, core.conv_pack_weights(c["w"].copy(), td), c["scale"], c["shift"], kernel, d, residual=res)
    dy, w, sc = _dev(c["dy"]), _dev(c["w"]), _dev(c["scale"])
    dx = cin % 32 == 0
    full = core.conv_bn_backward(x, w, sc, out, dy, kernel, d, want_features=dx, want_pre=True,
                                 grad_features_dtype=torch.float32, canary=GUARD)
    _guards_intact(full)
    assert set(full) == {n for n in NAMES if dx or n != "features"} | {"guards"}
    r = dict(out=out.cpu(), full=_cpu(full))
    if dx:
        a32 = core.conv_bn_backward(x, w, sc, out, dy, kernel, d, want_weight=False, want_scale=False, want_shift=False,
                                    features_add=add, grad_features_dtype=torch.float32, canary=GUARD)
        a16 = core.conv_bn_backward(x, w, sc, out, dy, kernel, d, want_weight=False, want_scale=False, want_shift=False,
                                    features_add=add, canary=GUARD)
        _guards_intact(a32), _guards_intact(a16)
        assert a16["features"].dtype == td and a32["features"].dtype == torch.float32
        r.update(add32=a32["features"].cpu(), add16=a16["features"].cpu())
    return r


@functools.lru_cache(maxsize=None)
def _reference(s, kernel, dtype, kind, with_add):
    """The reference on the device's own gh."""
    c, got = _inputs(s, kernel, kind), _run(s, kernel, dtype, kind)
    return cbr.backward(c["x"], c["w"], c["scale"], got["full"]["pre"], kernel, cbr.dilation_of(s, kernel), dtype,
                        add=c["add"] if with_add else None)


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("s, kernel, dtype", CASES, ids=IDS)
def test_masked_gradient_is_bitwise(s, kernel, dtype, kind):
    c, got = _inputs(s, kernel, kind), _run(s, kernel, dtype, kind)
    want = cbr.masked_gradient(c["dy"], got["out"], True, dtype)
    assert torch.equal(got["full"]["pre"].view(torch.int16), want.view(torch.int16))
    assert (got["out"] > 0).any() and (got["out"] == 0).any()                     # ReLU cuts some and not all


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s, kernel", [(1, 3), (5, 1), (9, 3), (11, 1)])
@pytest.mark.parametrize("out_f32, dy_half, relu", [(True, False, True), (False, True, True), (True, True, True),
                                                    (False, False, False), (False, True, False)])
def test_masked_gradient_for_every_dtype_of_out_and_dy(s, kernel, dtype, out_f32, dy_half, relu):
    c, td, d = cbr.random_inputs(s, kernel), cbr.DTYPES[dtype], cbr.dilation_of(s, kernel)
    x = _dev(c["x"], td)
    out = core.conv_bn(x, core.conv_pack_weights(c["w"].copy(), td), c["scale"], c["shift"], kernel, d, relu=relu,
                       out_dtype=torch.float32 if out_f32 else None)
    dy = _dev(c["dy"], td if dy_half else None)
    g = core.conv_bn_backward(x, _dev(c["w"]), c["scale"], out if relu else None, dy, kernel, d, relu=relu,
                              want_features=False, want_weight=False, want_scale=False, want_shift=True, want_pre=True,
                              canary=GUARD)
    _guards_intact(g)
    want = cbr.masked_gradient(dy.cpu(), out.cpu(), relu, dtype)
    assert torch.equal(g["pre"].cpu().view(torch.int16), want.view(torch.int16))
    r = cbr.backward(c["x"], c["w"], c["scale"], want, kernel, d, dtype)
    assert (np.abs(g["shift"].cpu().numpy().astype(np.float64) - r["dshift"]) <= r["tol_dshift"]).all()
    if not relu:
        assert (want.float() < 0).any() and not (want.float() == 0).all()


@pytest.mark.parametrize("s, kernel, dtype", CASES, ids=IDS)
def test_exact_inputs_give_the_float64_reference_bitwise(s, kernel, dtype):
    got, r = _run(s, kernel, dtype, "exact"), _reference(s, kernel, dtype, "exact", False)
    f = got["full"]
    for name, ref in (("weight", "dw"), ("scale", "dscale"), ("shift", "dshift"), ("features", "dx")):
        if name not in f:
            assert name == "features" and cbr.SHAPES[s][1] % 32
            continue
        bad = f[name].numpy().astype(np.float64) != r[ref].astype(np.float32).astype(np.float64)
        assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    assert np.array_equal(r["dw"].astype(np.float32).astype(np.float64), r["dw"])      # (dW itself is an fp32 value)
    assert (r["dw"] != 0).any() and (r["dshift"] != 0).any()
    if "add32" in got:
        ra = _reference(s, kernel, dtype, "exact", True)
        assert np.array_equal(got["add32"].numpy().astype(np.float64), ra["dx"])
        assert np.array_equal(ra["dx"].astype(np.float32).astype(np.float64), ra["dx"])


@pytest.mark.parametrize("s, kernel, dtype", CASES, ids=IDS)
def test_random_inputs_stay_within_the_bounds(s, kernel, dtype):
    """Measured on the MI355X: the table in DESIGN.md 10aa; the limits of 1 stand as derived."""
    got, r = _run(s, kernel, dtype, "random"), _reference(s, kernel, dtype, "random", False)
    f, worst = got["full"], {}
    for name, ref in (("features", "dx"), ("weight", "dw"), ("scale", "dscale"), ("shift", "dshift")):
        if name in f:
            worst[ref] = float((np.abs(f[name].numpy().astype(np.float64) - r[ref]) / r["tol_" + ref]).max())
    if "add32" in got:
        ra = _reference(s, kernel, dtype, "random", True)
        worst["dx+add"] = float((np.abs(got["add32"].numpy().astype(np.float64) - ra["dx"]) / ra["tol_dx"]).max())
    print("conv_bn_backward %s k%d %s: max err / tol %s" % (cbr.SHAPE_IDS[s], kernel, dtype,
                                                           " ".join("%s %.5f" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("s, kernel, dtype", [c for c in CASES if cbr.SHAPES[c[0]][1] % 32 == 0],
                         ids=[i for c, i in zip(CASES, IDS) if cbr.SHAPES[c[0]][1] % 32 == 0])
def test_half_dx_is_the_rne_conversion_of_the_fp32_dx(s, kernel, dtype, kind):
    """features_add is f18's residual operand: added in fp32 before the single final rounding."""
    got = _run(s, kernel, dtype, kind)
    want = got["add32"].to(cbr.DTYPES[dtype])
    assert torch.equal(got["add16"].view(torch.int16), want.view(torch.int16))
    assert not torch.equal(got["add32"], got["full"]["features"])              # (the add did something)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s, kernel", [(0, 3), (1, 1)])
def test_dx_is_refused_where_channels_in_is_no_multiple_of_32(s, kernel, dtype):
    c, td = cbr.random_inputs(s, kernel), cbr.DTYPES[dtype]
    x = _dev(c["x"], td)
    out = torch.ones((x.shape[0], cbr.SHAPES[s][2]) + tuple(x.shape[2:]), dtype=td, device=DEV)
    with pytest.raises(core.CoreError, match="channels_in % 32"):
        core.conv_bn_backward(x, _dev(c["w"]), c["scale"], out, out, kernel, cbr.dilation_of(s, kernel))


SUBSETS = [(1, 3, "float16"), (8, 1, "bfloat16"), (9, 3, "bfloat16"), (5, 1, "float16")]


@pytest.mark.parametrize("s, kernel, dtype", SUBSETS)
def test_every_choice_of_outputs_and_two_runs_give_the_same_bytes(s, kernel, dtype):
    c, td, d = cbr.random_inputs(s, kernel), cbr.DTYPES[dtype], cbr.dilation_of(s, kernel)
    first = _run(s, kernel, dtype, "random")
    x, out, dy, w, sc = _dev(c["x"], td), first["out"].to(DEV), _dev(c["dy"]), _dev(c["w"]), _dev(c["scale"])
    names = [n for n in NAMES if n in first["full"]]
    choices = [(n,) for n in names] + [("weight", "scale"), ("scale", "shift"), tuple(names)]
    if "features" in names:     # gh in the scratch (no "pre") beside the transposed pack, with and without the partials
        choices += [("features", "weight"), ("features", "shift")]
    for chosen in choices:
        want = {"want_" + n: n in chosen for n in NAMES}
        g = core.conv_bn_backward(x, w, sc, out, dy, kernel, d, grad_features_dtype=torch.float32, canary=GUARD, **want)
        _guards_intact(g)
        assert set(g) == set(chosen) | {"guards"}
        for n in chosen:
            a, b = g[n].cpu().contiguous(), first["full"][n].contiguous()
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (chosen, n)


def test_a_frame_alone_and_inside_a_batch():
    s, kernel, dtype = 9, 3, "bfloat16"                                        # three images, two chunks each
    c, td, d = cbr.random_inputs(s, kernel), cbr.DTYPES[dtype], cbr.dilation_of(s, kernel)
    got = _run(s, kernel, dtype, "random")
    x, out, dy = _dev(c["x"], td), got["out"].to(DEV), _dev(c["dy"])
    for f in (0, 2):
        g = core.conv_bn_backward(x[f:f + 1], _dev(c["w"]), c["scale"], out[f:f + 1], dy[f:f + 1], kernel, d,
                                  want_weight=False, want_scale=False, want_shift=False, want_pre=True,
                                  grad_features_dtype=torch.float32)
        assert torch.equal(g["pre"].cpu().view(torch.int16), got["full"]["pre"][f:f + 1].view(torch.int16))
        assert torch.equal(g["features"].cpu(), got["full"]["features"][f:f + 1])


@pytest.mark.parametrize("s, kernel, dtype", SUBSETS[:2])
def test_dy_is_read_in_place_at_an_image_stride(s, kernel, dtype):
    c, td, d = cbr.random_inputs(s, kernel), cbr.DTYPES[dtype], cbr.dilation_of(s, kernel)
    got = _run(s, kernel, dtype, "random")
    n, cin, cout, H, W, _ = cbr.SHAPES[s]
    wide = torch.full((max(n, 2), cout + 3, H, W), float("nan"), device=DEV)
    x = _dev(np.concatenate([c["x"]] * (max(n, 2) // n)), td)
    out = torch.cat([got["out"]] * (max(n, 2) // n)).to(DEV)
    wide[:, :cout] = _dev(np.concatenate([c["dy"]] * (max(n, 2) // n)))
    dy = wide[:, :cout]
    assert core._planes_in_place(dy, cout) and not dy.is_contiguous()
    dx = cin % 32 == 0
    a = core.conv_bn_backward(x, _dev(c["w"]), c["scale"], out, dy, kernel, d, want_features=dx, want_pre=True)
    b = core.conv_bn_backward(x, _dev(c["w"]), c["scale"], out, dy.contiguous(), kernel, d, want_features=dx, want_pre=True)
    for name in a:
        assert torch.equal(a[name].contiguous().view(torch.uint8), b[name].contiguous().view(torch.uint8)), name
    assert torch.isfinite(a["weight"]).all() and torch.isfinite(a["shift"]).all()


# ---- the training modules ----

def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and \
        torch.equal(a.detach().reshape(-1).view(torch.uint8), b.detach().reshape(-1).view(torch.uint8))


def _features(n, c, H, W, td, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, c, H, W, generator=g).abs()).to(DEV).to(td)


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv_bn_relu_module_equals_the_direct_calls(dtype):
    td = cbr.DTYPES[dtype]
    conv = torch.nn.Conv2d(32, 64, 3, padding=2, dilation=2, bias=False)
    bn = cb.batchnorm(64, 5).eval()
    layer = training.ConvBnReLU(conv, bn).to(DEV)
    x = _features(2, 32, 9, 33, td, 1).requires_grad_(True)
    y = layer(x)
    assert _bits_equal(y, cnn.ConvBnRelu(conv, bn, dtype=td, device=DEV)(x.detach()))          # the inference class
    gy = _features(2, 64, 9, 33, td, 2) - 0.5
    y.backward(gy)
    scale, shift = (t.to(DEV) for t in cnn.fold_batchnorm(bn))
    g = core.conv_bn_backward(x.detach(), layer.weight, scale, y.detach(), gy, 3, 2)
    assert _bits_equal(x.grad, g["features"]) and _bits_equal(layer.weight.grad, g["weight"])
    # (dscale, dshift) sent on through the fold in float64, rounded once
    inv = 1.0 / torch.sqrt(bn.running_var.double().to(DEV) + bn.eps)
    want_w = ((g["scale"].double() - g["shift"].double() * bn.running_mean.double().to(DEV)) * inv)
    assert torch.allclose(layer.bn.weight.grad.double(), want_w, rtol=2.0 ** -22, atol=0)
    assert _bits_equal(layer.bn.bias.grad, g["shift"])
    # frozen features: no dX launch, the same parameter gradients
    layer.zero_grad()
    layer(x.detach()).backward(gy)
    assert _bits_equal(layer.weight.grad, g["weight"]) and _bits_equal(layer.bn.bias.grad, g["shift"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cin, downsample, residual", [(32, True, True), (64, False, True), (32, True, False)])
def test_basic_block_module_equals_the_direct_calls(cin, downsample, residual, dtype):
    td = cbr.DTYPES[dtype]
    ref = cb.Block(cin, 64, dilation=(2, 2), downsample=downsample, residual=residual, seed=11).eval()
    block = training.BasicBlock(ref).to(DEV)
    x = _features(2, cin, 9, 33, td, 3).requires_grad_(True)
    y = block(x)
    assert _bits_equal(y, cnn.ResidualBlock(ref, dtype=td, device=DEV)(x.detach()))
    gy = _features(2, 64, 9, 33, td, 4) - 0.5
    y.backward(gy)
    # the same backward by hand: conv2, the downsample, conv1 with the second path joined inside its launch
    xd = x.detach()
    f1, f2 = [[t.to(DEV) for t in cnn.fold_batchnorm(b)] for b in (ref.bn1, ref.bn2)]
    y1 = core.conv_bn(xd, core.conv_pack_weights(block.weight1.detach(), td), f1[0], f1[1], 3, 2)
    g2 = core.conv_bn_backward(y1, block.weight2, f2[0], y.detach(), gy, 3, 2, want_pre=residual)
    add = None
    if residual and downsample:
        fd = [t.to(DEV) for t in cnn.fold_batchnorm(ref.downsample[1])]
        gd = core.conv_bn_backward(xd, block.weight_down, fd[0], None, g2["pre"], 1, 1, relu=False)
        add = gd["features"]
        assert _bits_equal(block.weight_down.grad, gd["weight"]) and _bits_equal(block.bn_down.bias.grad, gd["shift"])
    elif residual:
        add = g2["pre"]
    g1 = core.conv_bn_backward(xd, block.weight1, f1[0], y1, g2["features"], 3, 2, features_add=add)
    assert _bits_equal(x.grad, g1["features"])
    assert _bits_equal(block.weight1.grad, g1["weight"]) and _bits_equal(block.weight2.grad, g2["weight"])
    assert _bits_equal(block.bn1.bias.grad, g1["shift"]) and _bits_equal(block.bn2.bias.grad, g2["shift"])
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in block.parameters())


# ---- the whole modules against float64 autograd, on a family whose every intermediate is exact ----

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


def _exact_block(cin, downsample, residual, seed):
    ref = cb.Block(cin, 64, dilation=(2, 2), downsample=downsample, residual=residual, seed=seed)
    g = torch.Generator().manual_seed(seed)
    ref.bn1, ref.bn2 = _exact_bn(64, g), _exact_bn(64, g)
    _sparse_weight(ref.conv1, g), _sparse_weight(ref.conv2, g)
    if downsample:
        ref.downsample[1] = _exact_bn(64, g)
        _sparse_weight(ref.downsample[0], g)
    return ref.eval()


def _grads_equal_bitwise(named_dev, named_ref):
    for name, got in named_dev.items():
        want = named_ref[name].to(got.dtype)                      # torch's conversion on the CPU: round to nearest even
        assert _bits_equal(got.cpu(), want) or torch.equal(got.cpu().double(), want.double()), name   # (-0 == +0)
        assert float(want.double().abs().max()) > 0, name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cin, downsample, residual", [(32, True, True), (64, False, True), (32, True, False),
                                                       (64, False, False)])
def test_basic_block_equals_float64_autograd_on_exact_inputs(cin, downsample, residual, dtype):
    """Independent of how the backward composes its calls: float64 torch.autograd of conv_bn_reference.Block.  The
    family: x in {0, 1}, sparse weights in {-1, 0, 1}, BatchNorm with variance + eps = 1 and integer mean, weight (+-1)
    and bias, dY integers in [-2, 2].  Every intermediate is then a small integer that both half dtypes hold (checked
    below for conv1's output and its gradient, the two that are stored as halves), no ReLU mask can flip, and every
    gradient -- the input's, the three weights', every BatchNorm weight's and bias's -- must equal the float64 one, the
    input's after its one rounding to the half."""
    td = cbr.DTYPES[dtype]
    ref = _exact_block(cin, downsample, residual, seed=31)
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, 2, (2, cin, 9, 33), generator=g).float()
    dy = torch.randint(-2, 3, (2, 64, 9, 33), generator=g).float()
    block = training.BasicBlock(ref).to(DEV)
    xd = x.to(DEV).to(td).requires_grad_(True)
    y = block(xd)
    y.backward(dy.to(DEV).to(td))
    # float64 autograd of the reference's module
    r64 = ref.double()
    x64 = x.double().requires_grad_(True)
    y1 = torch.relu(r64.bn1(r64.conv1(x64)))
    y1.retain_grad()
    out = r64.bn2(r64.conv2(y1))
    if residual:
        out = out + (r64.downsample(x64) if downsample else x64)
    out = torch.relu(out)
    out.backward(dy.double())
    for t in (y1.detach(), y1.grad):                              # the two intermediates that are stored as halves
        assert torch.equal(t.to(td).double(), t)
    assert torch.equal(y.detach().cpu().double(), out.detach().to(td).double())
    assert (y1.detach() > 0).any() and (y1.detach() == 0).any() and (out.detach() == 0).any()
    dev = {"x": xd.grad, "weight1": block.weight1.grad, "weight2": block.weight2.grad,
           "bn1.weight": block.bn1.weight.grad, "bn1.bias": block.bn1.bias.grad,
           "bn2.weight": block.bn2.weight.grad, "bn2.bias": block.bn2.bias.grad}
    want = {"x": x64.grad, "weight1": r64.conv1.weight.grad, "weight2": r64.conv2.weight.grad,
            "bn1.weight": r64.bn1.weight.grad, "bn1.bias": r64.bn1.bias.grad,
            "bn2.weight": r64.bn2.weight.grad, "bn2.bias": r64.bn2.bias.grad}
    if downsample and residual:
        dev.update({"weight_down": block.weight_down.grad, "bn_down.weight": block.bn_down.weight.grad,
                    "bn_down.bias": block.bn_down.bias.grad})
        want.update({"weight_down": r64.downsample[0].weight.grad, "bn_down.weight": r64.downsample[1].weight.grad,
                     "bn_down.bias": r64.downsample[1].bias.grad})
    assert len(dev) == len(list(block.parameters())) + 1
    _grads_equal_bitwise(dev, want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv_bn_relu_module_equals_float64_autograd_on_exact_inputs(dtype):
    td = cbr.DTYPES[dtype]
    g = torch.Generator().manual_seed(8)
    conv = torch.nn.Conv2d(32, 64, 3, padding=4, dilation=4, bias=False)
    _sparse_weight(conv, g)
    bn = _exact_bn(64, g)
    x = torch.randint(0, 2, (2, 32, 9, 33), generator=g).float()
    dy = torch.randint(-2, 3, (2, 64, 9, 33), generator=g).float()
    layer = training.ConvBnReLU(conv, bn).to(DEV)
    xd = x.to(DEV).to(td).requires_grad_(True)
    layer(xd).backward(dy.to(DEV).to(td))
    conv64, bn64 = conv.double(), bn.double()
    x64 = x.double().requires_grad_(True)
    torch.relu(bn64(conv64(x64))).backward(dy.double())
    _grads_equal_bitwise({"x": xd.grad, "weight": layer.weight.grad, "bn.weight": layer.bn.weight.grad,
                          "bn.bias": layer.bn.bias.grad},
                         {"x": x64.grad, "weight": conv64.weight.grad, "bn.weight": bn64.weight.grad,
                          "bn.bias": bn64.bias.grad})


def test_a_training_step_gives_the_same_gradients_on_two_runs():
    td = torch.bfloat16
    torch.manual_seed(7)
    n, H, W = 2, 9, 33

    def pair(c, d):
        return torch.nn.Conv2d(c, c, 3, padding=d, dilation=d, bias=False), cb.batchnorm(c, 20 + d).eval()

    net = torch.nn.ModuleList([training.BasicBlock(cb.Block(32, 64, dilation=(2, 2), downsample=True, seed=3).eval()),
                               training.ConvBnReLU(*pair(64, 2)), training.ConvBnReLU(*pair(64, 1)),
                               training.SegmentationHead(64, 5, 2)]).to(DEV)
    x = _features(n, 32, H, W, td, 9)
    g = torch.Generator().manual_seed(4)
    target = torch.randint(0, 5, (n, H, W), generator=g).to(torch.uint8)
    target[0, :2] = 255
    ids = torch.randint(0, 4, (n, H, W), generator=g, dtype=torch.int32) * 1000
    nll, off = training.SemanticNLLLoss(n_classes=5), training.OffsetLossSL()

    def step():
        net.zero_grad()
        f = x
        for m in net:
            f = m(f)
        loss = nll(f, target.to(DEV)) + off(f[:, 5:7], ids.to(DEV))
        loss.backward()
        return [loss.detach().clone()] + [p.grad.clone() for p in net.parameters()]

    first, second = step(), step()
    assert len(first) == 1 + 9 + 3 + 3 + 2
    for a, b in zip(first, second):
        assert torch.isfinite(a).all() and _bits_equal(a, b)
    assert all(float(t.abs().max()) > 0 for t in first[1:])
