"""The downsampling layers' launches (f19) on the device against tests/conv_stride_reference.py, pinned as f17 and f18
are: inputs whose arithmetic is exact in every order must give the float64 reference bit for bit, and random inputs
must stay within the derived bound tol = |scale| taps channels_in 2^-23 sum|w x| + ulp_fp32(pre-residual) [+
ulp_fp32(pre-ReLU)], which does not depend on the stride; each bound test prints max(err / tol).  Every shape runs at
stride 2 as a 3x3 and as a 1x1 convolution, with and without a residual, in both dtypes.  Then: relu = 0, the half output
as the RNE conversion of the same call's fp32 output, guards behind the output and around the INPUT (a load outside the
image would change the result; nothing is provoked), determinism, batch invariance, stride 1 as core.conv_bn's bytes,
cnn.StridedResidualBlock against the composed calls and cnn.DrnDownsampling in front of the DP."""
import functools

import numpy as np
import pytest
import torch

import conv_bn_reference as cb
import conv_stride_reference as cs
from guards import check_guards
import helpers
from instance_stixels_amd import cnn, core

pytestmark = pytest.mark.gpu

DTYPES = sorted(cs.DTYPES)
Block = cb.Block
CASES = [(s, k, res, dt) for s in range(len(cs.SHAPES)) for k in cs.KERNELS for res in (False, True) for dt in DTYPES]
IDS = ["%s-k%d-%s-%s" % (cs.SHAPE_IDS[s], k, "res" if res else "plain", dt) for s, k, res, dt in CASES]
RES_CASES = [c for c in CASES if c[2]]
RES_IDS = [i for c, i in zip(CASES, IDS) if c[2]]
GUARD = 64
DEV = torch.device("cuda", 0)


def _inputs(s, kernel, kind):
    return cs.exact_inputs(s, kernel) if kind == "exact" else cs.random_inputs(s, kernel)


def _operands(s, kernel, with_res, dtype, kind):
    c, td = _inputs(s, kernel, kind), cs.DTYPES[dtype]
    x = torch.from_numpy(c["x"].copy()).to(DEV).to(td)
    res = torch.from_numpy(c["res"].copy()).to(DEV).to(td) if with_res else None
    return c, x, res, core.conv_pack_weights(c["w"].copy(), td)


@functools.lru_cache(maxsize=None)
def _run(s, kernel, with_res, dtype, kind, relu=True):
    """One guarded call with fp32 output and one with half output, on the same device operands."""
    c, x, res, packed = _operands(s, kernel, with_res, dtype, kind)
    f32, g32 = core.conv_bn_stride(x, packed, c["scale"], c["shift"], kernel, 2, residual=res, relu=relu,
                                   out_dtype=torch.float32, canary=GUARD)
    half, g16 = core.conv_bn_stride(x, packed, c["scale"], c["shift"], kernel, 2, residual=res, relu=relu,
                                    canary=GUARD)
    assert half.dtype == cs.DTYPES[dtype] and f32.dtype == torch.float32
    return dict(f32=f32.cpu().numpy(), half=half.cpu(), guards=(g32["out"], g16["out"]))


def _out_shape(s):
    n, cin, cout, H, W = cs.SHAPES[s]
    return (n, cout, (H + 1) // 2, (W + 1) // 2)


@pytest.mark.parametrize("s, kernel, with_res, dtype", CASES, ids=IDS)
def test_exact_inputs_give_the_float64_reference_bitwise(s, kernel, with_res, dtype):
    got, ref = _run(s, kernel, with_res, dtype, "exact")["f32"], cs.exact_reference(s, kernel, with_res)["ref"]
    assert got.shape == _out_shape(s)
    bad = got.astype(np.float64) != ref                          # (every value of ref is an fp32 value; -0 == +0)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5].tolist())
    assert (ref > 0).any() and (ref == 0).any()


@pytest.mark.parametrize("s, kernel, with_res, dtype", CASES, ids=IDS)
def test_random_inputs_stay_within_the_bound(s, kernel, with_res, dtype):
    """Measured on the MI355X: the table in DESIGN.md 10y; the limit of 1 stands as derived."""
    got, r = _run(s, kernel, with_res, dtype, "random")["f32"], cs.random_reference(s, kernel, dtype, with_res)
    assert got.shape == _out_shape(s)
    ratio = np.abs(got.astype(np.float64) - r["ref"]) / r["tol"]
    print("conv_bn_stride %s k%d %s %s: max err / tol %.5f" % (cs.SHAPE_IDS[s], kernel, "res" if with_res else "plain",
                                                               dtype, float(ratio.max())))
    assert ratio.max() <= 1.0, float(ratio.max())
    assert (r["ref"] > 0).any() and (r["ref"] == 0).any()        # ReLU cuts some and not all


@pytest.mark.parametrize("s, kernel, with_res, dtype", RES_CASES, ids=RES_IDS)
def test_without_relu_with_a_residual(s, kernel, with_res, dtype):
    got = _run(s, kernel, True, dtype, "random", relu=False)["f32"]
    r = cs.random_reference(s, kernel, dtype, True, relu=False)
    ratio = np.abs(got.astype(np.float64) - r["ref"]) / r["tol"]
    print("conv_bn_stride %s k%d res %s relu=0: max err / tol %.5f" % (cs.SHAPE_IDS[s], kernel, dtype,
                                                                       float(ratio.max())))
    assert ratio.max() <= 1.0, float(ratio.max())
    assert (got < 0).any()
    e = _run(s, kernel, True, dtype, "exact", relu=False)["f32"]
    assert np.array_equal(e.astype(np.float64), cs.exact_reference(s, kernel, True, relu=False)["ref"])
    assert (e < 0).any()


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("s, kernel, with_res, dtype", CASES, ids=IDS)
def test_half_output_is_the_rne_conversion_of_the_fp32_output(s, kernel, with_res, dtype, kind):
    got = _run(s, kernel, with_res, dtype, kind)
    want = torch.from_numpy(got["f32"]).to(cs.DTYPES[dtype])      # torch's conversion on the CPU: round to nearest even
    assert torch.equal(got["half"].view(torch.int16), want.view(torch.int16))
    if kind == "random":
        assert not torch.equal(want.float(), torch.from_numpy(got["f32"]))   # (the rounding did something)


@pytest.mark.parametrize("s, kernel, with_res, dtype", CASES, ids=IDS)
def test_guards_are_intact(s, kernel, with_res, dtype):
    for kind in ("exact", "random"):
        check_guards(dict(enumerate(_run(s, kernel, with_res, dtype, kind)["guards"])), GUARD, where=kind)


def _embedded(t, value):
    """A contiguous view with t's values inside a larger allocation whose surroundings hold +-value: a whole frame of
    them, and at least 4096 elements, in front and behind."""
    margin = max(4096, int(t[0].numel()))
    big = torch.full((t.numel() + 2 * margin,), value, dtype=t.dtype, device=t.device)
    big[1::2] = -value
    inner = big[margin:margin + t.numel()].view(t.shape)
    inner.copy_(t)
    assert inner.is_contiguous() and inner.data_ptr() == big.data_ptr() + margin * t.element_size()
    return big, inner


@pytest.mark.parametrize("s, kernel, with_res, dtype", CASES, ids=IDS)
def test_large_values_around_the_input_do_not_change_the_result(s, kernel, with_res, dtype):
    """The features (and the residual) inside larger allocations filled with +-32768: a load from outside the image
    that reached a sum would change it by thousands.  The clamped loads of the zero-filled border stay inside."""
    first = _run(s, kernel, with_res, dtype, "random")
    c, x, res, packed = _operands(s, kernel, with_res, dtype, "random")
    keep_x, x_in = _embedded(x, 32768.0)
    keep_res, res_in = _embedded(res, 32768.0) if with_res else (None, None)
    got = core.conv_bn_stride(x_in, packed, c["scale"], c["shift"], kernel, 2, residual=res_in, out_dtype=torch.float32)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), first["f32"].view(np.uint32))
    assert torch.equal(x_in, x) and abs(float(keep_x[0])) == 32768.0 and abs(float(keep_x[-1])) == 32768.0


@pytest.mark.parametrize("s, kernel, dtype", [(2, 3, "float16"), (5, 1, "bfloat16"), (7, 3, "bfloat16"), (6, 1, "float16"),
                                               (5, 3, "float16")])
def test_two_runs_give_equal_bytes(s, kernel, dtype):
    first = _run(s, kernel, True, dtype, "random")
    c, x, res, packed = _operands(s, kernel, True, dtype, "random")
    for out_dtype, key in ((torch.float32, "f32"), (None, "half")):
        again = core.conv_bn_stride(x, packed, c["scale"], c["shift"], kernel, 2, residual=res, out_dtype=out_dtype).cpu()
        want = first[key] if key == "half" else torch.from_numpy(first[key])
        assert again.view(torch.uint8).numpy().tobytes() == want.view(torch.uint8).numpy().tobytes()


@pytest.mark.parametrize("kernel", cs.KERNELS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s", [0, 3])
def test_a_frame_alone_equals_the_frame_in_a_batch(s, dtype, kernel):
    assert cs.SHAPES[s][0] > 1
    batch = _run(s, kernel, True, dtype, "random")
    c, x, res, packed = _operands(s, kernel, True, dtype, "random")
    for f in range(cs.SHAPES[s][0]):
        alone = core.conv_bn_stride(x[f:f + 1].clone(), packed, c["scale"], c["shift"], kernel, 2,
                                    residual=res[f:f + 1].clone(), out_dtype=torch.float32)
        assert np.array_equal(alone.cpu().numpy().view(np.uint32)[0], batch["f32"].view(np.uint32)[f])


@pytest.mark.parametrize("s, kernel, dtype", [(1, 3, "float16"), (2, 1, "bfloat16"), (5, 3, "bfloat16"), (2, 3, "float16"),
                                               (5, 1, "float16")])
def test_stride_1_gives_conv_bns_bytes(s, kernel, dtype):
    """f18's shapes and inputs through the new entry point at stride 1: the same launch, with a residual tensor, with
    the features as residual (channels_in = channels_out) and without."""
    n, cin, cout, H, W, _ = cb.SHAPES[s]
    td, d = cb.DTYPES[dtype], cb.dilation_of(s, kernel)
    c = cb.random_inputs(s, kernel)
    x = torch.from_numpy(c["x"].copy()).to(DEV).to(td)
    res = torch.from_numpy(c["res"].copy()).to(DEV).to(td)
    packed = core.conv_pack_weights(c["w"].copy(), td)
    residuals = [None, res] + ([x] if cin == cout else [])
    for residual in residuals:
        for out_dtype in (torch.float32, None):
            for relu in (True, False):
                old = core.conv_bn(x, packed, c["scale"], c["shift"], kernel, d, residual=residual, relu=relu,
                                   out_dtype=out_dtype)
                new = core.conv_bn_stride(x, packed, c["scale"], c["shift"], kernel, 1, d, residual=residual, relu=relu,
                                          out_dtype=out_dtype)
                assert old.dtype == new.dtype and old.shape == new.shape
                assert torch.equal(old.view(torch.uint8), new.view(torch.uint8))
    assert len(residuals) == (3 if s == 2 else 2)


# ---- cnn.StridedResidualBlock and cnn.DrnDownsampling ----

def _within_bound(name, dtype, got32, inp, conv, fold, kernel, stride, residual=None, relu=True):
    """One launch against the reference evaluated on the device's own inputs of that launch."""
    args = (inp.float().cpu().numpy(), conv.weight.detach().numpy(), fold[0].numpy(), fold[1].numpy(), kernel)
    res = None if residual is None else residual.float().cpu().numpy()
    r = cs.reference(*args, dtype, residual=res, relu=relu, stride=stride)
    assert got32.shape == r["ref"].shape
    ratio = np.abs(got32.cpu().numpy().astype(np.float64) - r["ref"]) / r["tol"]
    print("conv_bn_stride block %s %s: max err / tol %.5f" % (name, dtype, float(ratio.max())))
    assert ratio.max() <= 1.0, (name, float(ratio.max()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows, cols", [(9, 37), (16, 64)])
def test_strided_residual_block_equals_the_composed_calls(rows, cols, dtype):
    td = cs.DTYPES[dtype]
    block = Block(32, 64, dilation=(1, 1), downsample=True, stride=2, seed=70).eval()
    x = torch.randn(2, 32, rows, cols, generator=torch.Generator().manual_seed(71)).to(DEV).to(td)
    f1, f2, fd = (cnn.fold_batchnorm(bn) for bn in (block.bn1, block.bn2, block.downsample[1]))
    p1, p2, pd = (core.conv_pack_weights(conv.weight, td) for conv in (block.conv1, block.conv2, block.downsample[0]))
    y = core.conv_bn_stride(x, p1, *f1, 3, 2)
    res = core.conv_bn_stride(x, pd, *fd, 1, 2, relu=False)
    out_shape = (2, 64, (rows + 1) // 2, (cols + 1) // 2)
    assert tuple(y.shape) == tuple(res.shape) == out_shape and res.dtype == td and (res.float() < 0).any()
    want = core.conv_bn_stride(y, p2, *f2, 3, 1, residual=res)
    want32 = core.conv_bn_stride(y, p2, *f2, 3, 1, residual=res, out_dtype=torch.float32)

    rb = cnn.StridedResidualBlock(block, dtype=td)
    got = rb(x)
    assert got.dtype == td and tuple(got.shape) == out_shape and len(rb.packed) == 3
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert torch.equal(rb(x, out_dtype=torch.float32).view(torch.int32), want32.view(torch.int32))
    _within_bound("conv1", dtype, core.conv_bn_stride(x, p1, *f1, 3, 2, out_dtype=torch.float32), x, block.conv1, f1, 3, 2)
    _within_bound("downsample", dtype, core.conv_bn_stride(x, pd, *fd, 1, 2, relu=False, out_dtype=torch.float32), x,
                  block.downsample[0], fd, 1, 2, relu=False)
    _within_bound("conv2", dtype, want32, y, block.conv2, f2, 3, 1, residual=res)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["downsample", "identity"])
def test_strided_residual_block_at_stride_1_equals_residual_block(form, dtype):
    td = cs.DTYPES[dtype]
    cin, cout = (32, 64) if form == "downsample" else (32, 32)
    block = Block(cin, cout, dilation=(2, 4), downsample=form == "downsample", seed=72).eval()
    x = torch.randn(2, cin, 9, 37, generator=torch.Generator().manual_seed(73)).to(DEV).to(td)
    old, new = cnn.ResidualBlock(block, dtype=td), cnn.StridedResidualBlock(block, dtype=td)
    for out_dtype in (None, torch.float32):
        a, b = old(x, out_dtype=out_dtype), new(x, out_dtype=out_dtype)
        assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert len(old.packed) == len(new.packed) == (3 if form == "downsample" else 2)


def _seq_layer(cin, cout, dilation, seed, stride=1):
    g = torch.Generator().manual_seed(seed)
    conv = torch.nn.Conv2d(cin, cout, 3, stride=stride, padding=dilation, dilation=dilation, bias=False)
    bn = torch.nn.BatchNorm2d(cout)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / (9 * cout)) ** 0.5)
        bn.running_mean.copy_(torch.randn(cout, generator=g) * 0.2)
        bn.running_var.copy_(torch.rand(cout, generator=g) + 0.5)
        bn.weight.copy_(torch.rand(cout, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(cout, generator=g) * 0.1)
    return torch.nn.Sequential(conv, bn, torch.nn.ReLU()).eval()


def _model():
    """drn_d_22 from layer2 on with narrow dilated layers: the strides, dilations and block counts of the reference."""
    layers = dict(
        layer2=_seq_layer(16, 32, 1, seed=80, stride=2),
        layer3=[Block(32, 64, (1, 1), downsample=True, stride=2, seed=81).eval(), Block(64, 64, (1, 1), seed=85).eval()],
        layer4=[Block(64, 128, (1, 1), downsample=True, stride=2, seed=89).eval(), Block(128, 128, (1, 1), seed=93).eval()],
        layer5=[Block(128, 64, (2, 2), downsample=True, seed=40).eval(), Block(64, 64, (2, 2), seed=44).eval()],
        layer6=[Block(64, 32, (4, 4), downsample=True, seed=48).eval(), Block(32, 32, (4, 4), seed=52).eval()],
        layer7=_seq_layer(32, 64, 2, seed=7), layer8=_seq_layer(64, 32, 1, seed=8))
    seg = torch.nn.Conv2d(32, 21, 1, bias=True)
    with torch.no_grad():
        seg.weight.normal_(0, (2.0 / 21) ** 0.5, generator=torch.Generator().manual_seed(9))
        seg.bias.zero_()
    return layers, seg


def _by_hand(layers, x, td):
    """layer2, layer3 and layer4 launch by launch through core.conv_bn_stride: layer4's output."""
    conv, bn = layers["layer2"][0], layers["layer2"][1]
    y = core.conv_bn_stride(x, core.conv_pack_weights(conv.weight, td), *cnn.fold_batchnorm(bn), 3, 2)
    for block in layers["layer3"] + layers["layer4"]:
        s = block.conv1.stride[0]
        h = core.conv_bn_stride(y, core.conv_pack_weights(block.conv1.weight, td), *cnn.fold_batchnorm(block.bn1), 3, s)
        res = y if block.downsample is None else core.conv_bn_stride(
            y, core.conv_pack_weights(block.downsample[0].weight, td), *cnn.fold_batchnorm(block.downsample[1]), 1, s,
            relu=False)
        y = core.conv_bn_stride(h, core.conv_pack_weights(block.conv2.weight, td), *cnn.fold_batchnorm(block.bn2), 3, 1,
                                residual=res)
    return y


@pytest.mark.parametrize("dtype", DTYPES)
def test_drn_downsampling_equals_the_composed_calls_and_feeds_the_dp(dtype, monkeypatch):
    td = cs.DTYPES[dtype]
    case = helpers.build_case("drn_d_22_unary", 128, 256, 32, seed=3)
    cfg = case["cfg"]
    Hs, Ws, P2S = cfg.rows // 8, cfg.realcols, case["segmentation"].shape[-1]
    assert (Hs, Ws, P2S) == (16, 32, 32) and case["segmentation"].shape[2] == 21
    layers, seg = _model()
    x = torch.randn(1, 16, 128, 256, generator=torch.Generator().manual_seed(10)).abs().to(DEV).to(td)

    y = _by_hand(layers, x, td)
    assert y.dtype == td and tuple(y.shape) == (1, 128, Hs, Ws) and (y > 0).any()
    dilated = cnn.DrnDilated(layers["layer5"], layers["layer6"], layers["layer7"], layers["layer8"], seg, 19, P2S, dtype=td)
    want_seg, want_cnn = dilated.forward(y, want_cnn_out=True)

    net = cnn.DrnDownsampling(**layers, seg=seg, n_classes=19, rows_power2_segmentation=P2S, dtype=td)
    assert len(net.blocks) == 4 and len(net.dilated.blocks) == 4
    packed = [net.layer2.packed] + [p for b in net.blocks + net.dilated.blocks for p in b.packed] + \
             [layer.packed for layer in net.dilated.tail.layers]
    assert len(packed) == 23 and net.launches == 24               # 23 convolutions and the head
    launches = []
    for name in ("conv_bn_stride", "conv_bn", "conv3x3_bn_relu", "segmentation_head"):
        def counted(*args, _fn=getattr(core, name), _name=name, **kwargs):
            launches.append(_name)
            return _fn(*args, **kwargs)
        monkeypatch.setattr(core, name, counted)
    got_seg, got_cnn = net.forward(x, want_cnn_out=True)
    assert launches == ["conv_bn_stride"] * 23 + ["segmentation_head"]
    assert torch.equal(got_seg, want_seg) and got_seg.dtype == torch.int32 and tuple(got_seg.shape) == (1, Ws, 21, P2S)
    assert torch.equal(got_cnn.view(torch.int32), want_cnn.view(torch.int32))
    assert torch.equal(net(x.float()), want_seg)                  # another floating dtype is converted first

    # the DP takes the network's output: Sections identical to the oracle's on the same int tensor
    case["segmentation"] = got_seg.cpu().numpy()
    ref = helpers.run_oracle(case)
    got = helpers.run_core(case, want_tables=False)
    errs = helpers.compare(ref, got, 0, cfg, check_tables=False)
    assert not errs, errs[:5]


@pytest.mark.parametrize("dtype", DTYPES)
def test_drn_downsampling_on_extents_that_are_no_multiple_of_8(dtype):
    """2 x 16 x 37 x 75: the extents go 19 x 38, 10 x 19, 5 x 10, ceil(. / 2) three times."""
    td = cs.DTYPES[dtype]
    layers, seg = _model()
    x = torch.randn(2, 16, 37, 75, generator=torch.Generator().manual_seed(11)).abs().to(DEV).to(td)
    y = _by_hand(layers, x, td)
    assert tuple(y.shape) == (2, 128, 5, 10)
    dilated = cnn.DrnDilated(layers["layer5"], layers["layer6"], layers["layer7"], layers["layer8"], seg, 19, 8, dtype=td)
    want_seg, want_cnn = dilated.forward(y, want_cnn_out=True)
    net = cnn.DrnDownsampling(**layers, seg=seg, n_classes=19, rows_power2_segmentation=8, dtype=td)
    got_seg, got_cnn = net.forward(x, want_cnn_out=True)
    assert tuple(got_cnn.shape) == (2, 21, 5, 10) and tuple(got_seg.shape) == (2, 10, 21, 8)
    assert torch.equal(got_seg, want_seg) and torch.equal(got_cnn.view(torch.int32), want_cnn.view(torch.int32))
