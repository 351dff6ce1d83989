"""The backward pass of the stem (f23) on the MI355X, for both gradient sources: every output against
tests/stem_backward_reference.py within the derived bounds (each stage pinned on the device's own previous stage), the
exact family bit for bit, every output alone against the full call, determinism, batch invariance of gh1 and gh0,
guards around every output and the scratch, the image inside 0xFF bytes, training.Stem against cnn.DrnStem and float64
autograd, and training.Drn against the inference classes and the hand-chained core calls.  The largest err / tol of a
run is printed per case (profiles/f23_stem_backward_gpu_tests.log)."""
import functools

import numpy as np
import pytest
import torch

from guards import check_guards
import stem_backward_reference as sbr
import stem_reference as sr
import test_conv_stride_backward_gpu as f22
from instance_stixels_amd import cnn, core, training

pytestmark = pytest.mark.gpu

DTYPES = sorted(sbr.DTYPES)
# (shape, channels_next, dtype): channels_next 0 is source (a), dY; otherwise source (b), layer2's masked gradient
CASES = [(s, 0, dt) for s in range(len(sbr.SHAPES)) for dt in DTYPES] + [(s, cn, dt) for s, cn in sbr.NEXT_CASES for dt in DTYPES]
CASE_IDS = ["%s-%s" % (sbr.SHAPE_IDS[s], dt) if cn == 0 else "%s-c%d-%s" % (sbr.SHAPE_IDS[s], cn, dt) for s, cn, dt in CASES]
BATCHES = [(c, i) for c, i in zip(CASES, CASE_IDS) if sbr.SHAPES[c[0]][0] > 1]
DEV = torch.device("cuda", 0)
GUARD = 64
OUTPUTS = ("weight0", "scale0", "shift0", "weight1", "scale1", "shift1")


def _inputs(s, dtype, kind):
    c = dict(sbr.exact_inputs(s) if kind == "exact" else sbr.random_inputs(s))
    if kind != "exact":
        c["lut"] = sr.input_table(dtype)
    return c


@functools.lru_cache(maxsize=None)
def _operands(s, dtype, kind):
    """The case on the device, with the forward's saved tensors: (arrays, image, lut, mid, out, dY)."""
    c, td = _inputs(s, dtype, kind), sbr.DTYPES[dtype]
    image = torch.from_numpy(c["image"].copy()).to(DEV)
    lut = torch.from_numpy(c["lut"].copy()).to(DEV).to(td)
    packed = core.stem_pack_weights(c["w0"], c["w1"], td, device=DEV)
    out, mid = core.stem(image, lut, packed, c["scale0"], c["shift0"], c["scale1"], c["shift1"], want_mid=True)
    dy = torch.from_numpy(c["dy"].copy()).to(DEV)
    return c, image, lut, mid, out, dy


@functools.lru_cache(maxsize=None)
def _source(s, cn, dtype, kind):
    """The gradient's source as keywords of core.stem_backward, on the device."""
    if cn == 0:
        return dict(grad_out=_operands(s, dtype, kind)[5])
    nx = sbr.next_inputs(s, cn, kind)
    return dict(grad_next=torch.from_numpy(nx["gh"].copy()).to(DEV).to(sbr.DTYPES[dtype]),
                weight_next=torch.from_numpy(nx["w"].copy()).to(DEV), scale_next=torch.from_numpy(nx["scale"].copy()).to(DEV))


def _call(s, cn, dtype, kind, image=None, **more):
    c, img, lut, mid, out, dy = _operands(s, dtype, kind)
    return core.stem_backward(img if image is None else image, lut, c["w0"], c["w1"], c["scale0"], c["scale1"], mid, out,
                              **_source(s, cn, dtype, kind), **more)


@functools.lru_cache(maxsize=None)
def _run(s, cn, dtype, kind):
    """One guarded call for everything."""
    return _call(s, cn, dtype, kind, want_pre=True, canary=GUARD)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _cpu(t):
    return t.detach().cpu()


def _worst(got, ref, tol):
    err = np.abs(np.asarray(got, np.float64) - ref)
    ratio = np.where(err == 0, 0.0, err / np.where(tol > 0, tol, np.finfo(np.float64).tiny))
    return float(ratio.max())


@pytest.mark.parametrize("s, cn, dtype", CASES, ids=CASE_IDS)
def test_random_inputs_stay_within_the_bounds(s, cn, dtype):
    """Measured on the MI355X: the table in DESIGN.md 10ac; the limit of 1 stands as derived."""
    c, image, lut, mid, out, dy = _operands(s, dtype, "random")
    got = _run(s, cn, dtype, "random")
    mid_h, out_h = _cpu(mid), _cpu(out)
    gh1, gh0 = _cpu(got["pre1"]), _cpu(got["pre0"])
    worst = {}
    assert (_bits(gh1)[out_h.float() <= 0] == 0).all()
    if cn == 0:
        # gh1: bit for bit the masked gradient of dY under the stored out
        assert torch.equal(_bits(gh1), _bits(sbr.masked_gradient(c["dy"], out_h, dtype)))
    else:
        # gh1 against the reference's g_out under the stored mask, within its bound plus the half ulp of the rounding:
        # what source (a) makes of the reference's g_out is round_half(ref) under the same mask, half an ulp from ref
        nx = sbr.next_inputs(s, cn, "random")
        gsrc = _cpu(_source(s, cn, dtype, "random")["grad_next"])
        r = sbr.next_gradient(gsrc, nx["w"], nx["scale"], c["dy"].shape, dtype)
        on = (out_h.float() > 0).numpy()
        worst["gout"] = _worst(gh1.double().numpy()[on], r["ref"][on], r["tol_half"][on]) if on.any() else 0.0
    # dMid from the device's gh1; gh0 is it where the stored mid > 0 and +0 elsewhere
    d = sbr.data_gradient(gh1, c["w1"], c["scale1"], dtype)
    active = (mid_h.float() > 0).numpy()
    assert (_bits(gh0).numpy()[~active] == 0).all()
    worst["dmid"] = _worst(gh0.double().numpy()[active], d["ref"][active], d["tol_half"][active]) if active.any() else 0.0
    # layer1's gradients from the device's gh1 and mid, layer0's from the device's gh0
    l1 = sbr.layer1_gradients(mid_h.float().numpy(), c["w1"], c["scale1"], gh1, dtype)
    l0 = sbr.layer0_gradients(c["image"], c["lut"], c["w0"], c["scale0"], gh0, dtype)
    for layer, r in ((0, l0), (1, l1)):
        for name, key in (("weight", "dw"), ("scale", "dscale"), ("shift", "dshift")):
            worst["%s%d" % (name, layer)] = _worst(_cpu(got["%s%d" % (name, layer)]).numpy(), r[key], r["tol_" + key])
    print("f23 err/tol %s c%d %s: %s" % (sbr.SHAPE_IDS[s], cn, dtype, " ".join("%s %.4f" % kv for kv in sorted(worst.items()))))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("s, cn, dtype", CASES, ids=CASE_IDS)
def test_exact_inputs_give_the_float64_reference_bitwise(s, cn, dtype):
    c, image, lut, mid, out, dy = _operands(s, dtype, "exact")
    got, ref = _run(s, cn, dtype, "exact"), sbr.exact_reference(s) if cn == 0 else sbr.exact_reference_next(s, cn)
    td = sbr.DTYPES[dtype]
    half = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(td)
    # the forward's saved tensors are the reference's
    assert torch.equal(_bits(_cpu(mid)), _bits(half(ref["mid"])))
    assert torch.equal(_bits(_cpu(out)), _bits(half(ref["out"])))
    # (x + 0.0: the reference's masked zeros may carry a sign; the device's are +0)
    assert torch.equal(_bits(_cpu(got["pre1"])), _bits(half(ref["gh1"] + 0.0)))
    assert torch.equal(_bits(_cpu(got["pre0"])), _bits(half(ref["gh0"] + 0.0)))
    for name, key in (("weight0", "dw0"), ("scale0", "dscale0"), ("shift0", "dshift0"), ("weight1", "dw1"),
                      ("scale1", "dscale1"), ("shift1", "dshift1")):
        want = torch.from_numpy(ref[key]).to(torch.float32)         # the float64 value rounded once
        # (by value: every value is finite, and a zero's sign is scale's times +0 on the device, torch's own here)
        assert torch.isfinite(_cpu(got[name])).all() and torch.equal(_cpu(got[name]), want), name


@pytest.mark.parametrize("s, cn, dtype", CASES, ids=CASE_IDS)
def test_every_output_alone_has_the_bytes_of_the_full_call(s, cn, dtype):
    full = _run(s, cn, dtype, "random")
    for name in OUTPUTS:
        alone = _call(s, cn, dtype, "random", **{"want_" + k: k == name for k in OUTPUTS})
        assert sorted(alone) == [name]
        assert torch.equal(alone[name].view(torch.int32), full[name].view(torch.int32)), name
    pre = _call(s, cn, dtype, "random", want_pre=True, **{"want_" + k: False for k in OUTPUTS})
    assert sorted(pre) == ["pre0", "pre1"]
    for name in ("pre0", "pre1"):
        assert torch.equal(_bits(pre[name]), _bits(full[name])), name


@pytest.mark.parametrize("s, cn, dtype", CASES, ids=CASE_IDS)
def test_two_runs_give_equal_bytes_and_a_half_dy_passes_through(s, cn, dtype):
    first = _run(s, cn, dtype, "random")
    again = _call(s, cn, dtype, "random", want_pre=True)
    for name in OUTPUTS:
        assert torch.equal(again[name].view(torch.int32), first[name].view(torch.int32)), name
    for name in ("pre0", "pre1"):
        assert torch.equal(_bits(again[name]), _bits(first[name])), name
    if cn:
        return
    # dY in the half dtype, read in place from a tensor with a larger batch stride: the bytes of its fp32 copy
    c, image, lut, mid, out, dy = _operands(s, dtype, "random")
    n, H, W = sbr.SHAPES[s]
    wide = torch.zeros((n, 20, H, W), dtype=sbr.DTYPES[dtype], device=DEV)
    wide[:, :16] = dy.to(sbr.DTYPES[dtype])
    half = core.stem_backward(image, lut, c["w0"], c["w1"], c["scale0"], c["scale1"], mid, out, grad_out=wide[:, :16],
                              want_pre=True)
    widened = core.stem_backward(image, lut, c["w0"], c["w1"], c["scale0"], c["scale1"], mid, out,
                                 grad_out=wide[:, :16].float(), want_pre=True)
    for name in OUTPUTS:
        assert torch.equal(half[name].view(torch.int32), widened[name].view(torch.int32)), name
    assert torch.equal(_bits(half["pre1"]), _bits(widened["pre1"])) and torch.equal(_bits(half["pre0"]), _bits(widened["pre0"]))


@pytest.mark.parametrize("s, cn, dtype", [c for c, i in BATCHES], ids=[i for c, i in BATCHES])
def test_a_frame_alone_equals_the_frame_in_a_batch(s, cn, dtype):
    batch = _run(s, cn, dtype, "random")
    c, image, lut, mid, out, dy = _operands(s, dtype, "random")
    src = _source(s, cn, dtype, "random")
    for f in range(sbr.SHAPES[s][0]):
        one_src = dict(src, grad_next=src["grad_next"][f:f + 1]) if cn else dict(grad_out=dy[f:f + 1])
        one = core.stem_backward(image[f:f + 1], lut, c["w0"], c["w1"], c["scale0"], c["scale1"], mid[f:f + 1],
                                 out[f:f + 1], **one_src, want_pre=True, want_weight0=False, want_scale0=False,
                                 want_shift0=False, want_weight1=False, want_scale1=False, want_shift1=False)
        for name in ("pre0", "pre1"):
            assert torch.equal(_bits(one[name][0]), _bits(batch[name][f])), (name, f)


@pytest.mark.parametrize("s, cn, dtype", CASES, ids=CASE_IDS)
def test_guards_are_intact(s, cn, dtype):
    for kind in ("exact", "random"):
        check_guards(_run(s, cn, dtype, kind)["guards"], GUARD, OUTPUTS + ("pre0", "pre1", "scratch"), where=kind)


@pytest.mark.parametrize("s, cn, dtype", CASES, ids=CASE_IDS)
def test_bytes_of_0xff_around_the_image_do_not_change_the_result(s, cn, dtype):
    """The image inside a larger allocation filled with 0xFF on both sides: a load from outside the image would index
    lut[c][255], about +3.8, and change a sum of G0.  The clamped loads of the zero-filled border stay inside."""
    first = _run(s, cn, dtype, "random")
    c, image, lut, mid, out, dy = _operands(s, dtype, "random")
    margin = 4096
    big = torch.full((image.numel() + 2 * margin,), 0xFF, dtype=torch.uint8, device=DEV)
    inner = big[margin:margin + image.numel()].view(image.shape)
    inner.copy_(image)
    assert inner.is_contiguous() and inner.data_ptr() == big.data_ptr() + margin
    got = _call(s, cn, dtype, "random", image=inner, want_pre=True)
    for name in OUTPUTS:
        assert torch.equal(got[name].view(torch.int32), first[name].view(torch.int32)), name
    assert torch.equal(inner, image) and int(big[0]) == 0xFF and int(big[-1]) == 0xFF
    assert float(lut[:, 255].float().min()) > 3.0


def _exact_layers(c):
    """layer0 and layer1 as modules whose folded BatchNorms are exactly the exact family's scales and shifts: weight =
    scale, bias = shift, running_mean 0, running_var 1 - eps."""
    layer0, layer1 = sr.stem_layers(0)
    with torch.no_grad():
        for layer, w, scale, shift in ((layer0, "w0", "scale0", "shift0"), (layer1, "w1", "scale1", "shift1")):
            layer[0].weight.copy_(torch.from_numpy(c[w]))
            bn = layer[1]
            bn.weight.copy_(torch.from_numpy(c[scale])), bn.bias.copy_(torch.from_numpy(c[shift]))
            bn.running_mean.zero_(), bn.running_var.fill_(1.0), setattr(bn, "eps", 0.0)
    return layer0, layer1


@pytest.mark.parametrize("dtype", DTYPES)
def test_training_stem_forward_is_drn_stem_bitwise(dtype):
    td = sbr.DTYPES[dtype]
    layer0, layer1 = sr.stem_layers(seed=60)
    image = torch.from_numpy(np.random.default_rng(61).integers(0, 256, (2, 19, 70, 3)).astype(np.uint8)).to(DEV)
    want = cnn.DrnStem(layer0, layer1, sr.MEAN, sr.STD, dtype=td, device=DEV)(image)
    stem = training.Stem(layer0, layer1, sr.MEAN, sr.STD, td).to(DEV)
    got = stem(image)
    assert got.requires_grad and torch.equal(_bits(got), _bits(want))
    # its backward is core.stem_backward's bytes, sent on through the folds by autograd
    dy = torch.randn(got.shape, generator=torch.Generator().manual_seed(62)).to(DEV)
    got.backward(dy)
    scale0, shift0 = stem.bn0.fold()
    scale1, shift1 = stem.bn1.fold()
    packed = core.stem_pack_weights(stem.weight0, stem.weight1, td, device=DEV)
    out, mid = core.stem(image, stem.lut, packed, scale0, shift0, scale1, shift1, want_mid=True)
    g = core.stem_backward(image, stem.lut, stem.weight0, stem.weight1, scale0, scale1, mid, out, grad_out=dy)
    assert torch.equal(stem.weight0.grad, g["weight0"]) and torch.equal(stem.weight1.grad, g["weight1"])
    for bn, scale, shift in ((stem.bn0, g["scale0"], g["shift0"]), (stem.bn1, g["scale1"], g["shift1"])):
        inv = 1.0 / torch.sqrt(bn.running_var.double() + bn.eps)
        assert torch.equal(bn.bias.grad, shift)
        want_w = (scale.double() * inv - shift.double() * bn.running_mean.double() * inv).float()
        assert torch.allclose(bn.weight.grad, want_w, rtol=1e-6, atol=0)
    assert all(p.grad is not None for p in stem.parameters())


@pytest.mark.parametrize("dtype", DTYPES)
def test_training_stem_gradients_are_float64_autograd_bitwise_on_the_exact_family(dtype):
    s = sbr.SHAPES.index((3, 33, 130))
    c, ref, td = sbr.exact_inputs(s), sbr.exact_reference(s), sbr.DTYPES[dtype]
    stem = training.Stem(*_exact_layers(c), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), td).to(DEV)
    with torch.no_grad():       # the family's table of {0, 1} in place of the normalisation's
        stem.lut.copy_(torch.from_numpy(c["lut"]).to(td))
    out = stem(torch.from_numpy(c["image"].copy()).to(DEV))
    out.backward(torch.from_numpy(c["dy"].copy()).to(DEV))
    a = sbr.autograd64(dict(c, w0=c["m0"], w1=c["m1"]), c["lut"].astype(np.float64))
    for p, key in ((stem.weight0, "dw0"), (stem.weight1, "dw1"), (stem.bn0.weight, "dscale0"), (stem.bn0.bias, "dshift0"),
                   (stem.bn1.weight, "dscale1"), (stem.bn1.bias, "dshift1")):
        assert np.array_equal(a[key], ref[key]), key                     # autograd is the reference here
        want = torch.from_numpy(a[key]).to(torch.float32)              # by value: a zero's sign is scale's on the device
        assert torch.isfinite(_cpu(p.grad)).all() and torch.equal(_cpu(p.grad), want), key


@pytest.mark.parametrize("dtype", DTYPES)
def test_drn_equals_the_inference_classes_and_the_hand_chained_calls(dtype):
    """The whole base with layer2 .. layer8 reduced to a width of 32 on 2 x 19 x 35 x 3 bytes, followed by
    SegmentationHead and SemanticNLLLoss: the forward is the inference classes' (cnn), every parameter has a gradient,
    and every gradient equals the core calls chained by hand from the gradient that reaches layer8's output, bit for
    bit; two steps give the same bytes."""
    td = sbr.DTYPES[dtype]
    layers = f22._reduced_layers()
    layer0, layer1 = sr.stem_layers(seed=70)
    net = training.Drn.from_base(torch.nn.Sequential(layer0, layer1, *layers), sr.MEAN, sr.STD, td).to(DEV)
    torch.manual_seed(11)
    head = training.SegmentationHead(32, 5, 2).to(DEV)
    nll = training.SemanticNLLLoss(n_classes=5)
    image = torch.from_numpy(np.random.default_rng(71).integers(0, 256, (2, 19, 35, 3)).astype(np.uint8)).to(DEV)
    target = torch.randint(0, 5, (2, 3, 5), generator=torch.Generator().manual_seed(4)).to(torch.uint8)
    target[0, :1] = 255

    def step():
        net.zero_grad(), head.zero_grad()
        out = net(image)
        out.retain_grad()
        nll(head(out), target.to(DEV)).backward()
        return out.detach(), out.grad.clone(), {n: p.grad.clone() if p.grad is not None else None for n, p in net.named_parameters()}

    out, gout, grads = step()
    assert tuple(out.shape) == (2, 32, 3, 5) and out.dtype == td
    assert all(g is not None and torch.isfinite(g).all() and g.any() for g in grads.values()), \
        [n for n, g in grads.items() if g is None or not g.any()]
    # the forward: the inference classes, launch for launch
    out1, mid = cnn.DrnStem(layer0, layer1, sr.MEAN, sr.STD, dtype=td, device=DEV)(image, want_mid=True)
    refs = [layers[0]] + [b for layer in layers[1:5] for b in layer] + layers[5:]
    f, saved = out1, []
    for ref in refs:
        saved.append(f)
        if isinstance(ref, torch.nn.Sequential):
            f = cnn.StridedConvBnRelu(ref[0], ref[1], dtype=td, device=DEV)(f)
        else:
            f = cnn.StridedResidualBlock(ref, dtype=td, device=DEV)(f)
    saved.append(f)
    assert f22._bits_equal(out, f)
    # the backward by hand, from layer8 down to layer3 as f22's test, then layer2 and the stem
    gy, seen, mods = gout, 0, net.layers.layers
    for i in reversed(range(1, len(refs))):
        ref, mod, xin, y = refs[i], mods[i], saved[i], saved[i + 1]
        prefix = "layers.layers.%d." % i
        if isinstance(ref, torch.nn.Sequential):
            conv, bn = ref[0], ref[1]
            scale = cnn.fold_batchnorm(bn)[0].to(DEV)
            gg = core.conv_bn_stride_backward(xin, mod.weight, scale, y, gy, 3, int(conv.stride[0]), int(conv.dilation[0]))
            want = {"weight": gg["weight"]}
            want["bn.weight"], want["bn.bias"] = f22._fold_grads(bn, gg["scale"], gg["shift"])
            gy = gg["features"]
        else:
            want, gy = f22._block_by_hand(ref, mod, xin, y, gy, td)
        for name, gw in want.items():
            assert f22._bits_equal(grads[prefix + name], gw), prefix + name
            seen += 1
    scale2 = cnn.fold_batchnorm(layers[0][1])[0].to(DEV)
    g2 = core.conv_bn_stride_backward(out1, mods[0].weight, scale2, saved[1], gy, 3, 2, want_features=False, want_pre=True)
    want = {"layers.layers.0.weight": g2["weight"]}
    want["layers.layers.0.bn.weight"], want["layers.layers.0.bn.bias"] = f22._fold_grads(layers[0][1], g2["scale"], g2["shift"])
    scale0, scale1 = (cnn.fold_batchnorm(layer[1])[0].to(DEV) for layer in (layer0, layer1))
    g = core.stem_backward(image, net.stem.lut, net.stem.weight0, net.stem.weight1, scale0, scale1, mid, out1,
                           grad_next=g2["pre"], weight_next=mods[0].weight, scale_next=scale2)
    want["stem.weight0"], want["stem.weight1"] = g["weight0"], g["weight1"]
    want["stem.bn0.weight"], want["stem.bn0.bias"] = f22._fold_grads(layer0[1], g["scale0"], g["shift0"])
    want["stem.bn1.weight"], want["stem.bn1.bias"] = f22._fold_grads(layer1[1], g["scale1"], g["shift1"])
    for name, gw in want.items():
        assert f22._bits_equal(grads[name], gw), name
        seen += 1
    assert seen == len(grads) == 6 + 3 + 3 * 9 + 5 * 6 + 2 * 3
    out2, gout2, grads2 = step()
    assert f22._bits_equal(out, out2) and f22._bits_equal(gout, gout2) and all(f22._bits_equal(grads[n], grads2[n]) for n in grads)
    # DrnLayers still refuses what it refused
    with pytest.raises(core.CoreError, match="requires grad: the stem is frozen"):
        net.layers(out1.clone().requires_grad_(True))
