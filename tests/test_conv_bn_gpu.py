"""The residual blocks' launches (f18) on the device against tests/conv_bn_reference.py, pinned as f17 is: inputs whose
arithmetic is exact in every order must give the float64 reference bit for bit, and random inputs must stay within the
derived bound tol = |scale| taps channels_in 2^-23 sum|w x| + ulp_fp32(pre-residual) [+ ulp_fp32(pre-ReLU)]; each bound
test prints max(err / tol).  Every shape runs as a 3x3 and as a 1x1 convolution, with and without a residual, in both
dtypes.  Then: relu = 0, the half output as the RNE conversion of the same call's fp32 output, guards, determinism,
batch invariance, the bytes of f17's entry points, the features as residual, cnn.ResidualBlock against the composed
calls and cnn.DrnDilated in front of the DP."""
import functools

import numpy as np
import pytest
import torch

import conv_bn_reference as cb
from guards import check_guards
import helpers
from instance_stixels_amd import cnn, core

pytestmark = pytest.mark.gpu

DTYPES = sorted(cb.DTYPES)
Block = cb.Block
CASES = [(s, k, res, dt) for s in range(len(cb.SHAPES)) for k in cb.KERNELS for res in (False, True) for dt in DTYPES]
IDS = ["%s-k%d-%s-%s" % (cb.SHAPE_IDS[s], k, "res" if res else "plain", dt) for s, k, res, dt in CASES]
RES_CASES = [c for c in CASES if c[2]]
RES_IDS = [i for c, i in zip(CASES, IDS) if c[2]]
GUARD = 64
DEV = torch.device("cuda", 0)


def _inputs(s, kernel, kind):
    return cb.exact_inputs(s, kernel) if kind == "exact" else cb.random_inputs(s, kernel)


def _operands(s, kernel, with_res, dtype, kind):
    c, td = _inputs(s, kernel, kind), cb.DTYPES[dtype]
    x = torch.from_numpy(c["x"].copy()).to(DEV).to(td)
    res = torch.from_numpy(c["res"].copy()).to(DEV).to(td) if with_res else None
    return c, x, res, core.conv_pack_weights(c["w"].copy(), td)


@functools.lru_cache(maxsize=None)
def _run(s, kernel, with_res, dtype, kind, relu=True):
    """One guarded call with fp32 output and one with half output, on the same device operands."""
    c, x, res, packed = _operands(s, kernel, with_res, dtype, kind)
    d = cb.dilation_of(s, kernel)
    f32, g32 = core.conv_bn(x, packed, c["scale"], c["shift"], kernel, d, residual=res, relu=relu,
                            out_dtype=torch.float32, canary=GUARD)
    half, g16 = core.conv_bn(x, packed, c["scale"], c["shift"], kernel, d, residual=res, relu=relu, canary=GUARD)
    assert half.dtype == cb.DTYPES[dtype] and f32.dtype == torch.float32
    return dict(f32=f32.cpu().numpy(), half=half.cpu(), guards=(g32["out"], g16["out"]))


@pytest.mark.parametrize("s, kernel, with_res, dtype", CASES, ids=IDS)
def test_exact_inputs_give_the_float64_reference_bitwise(s, kernel, with_res, dtype):
    got, ref = _run(s, kernel, with_res, dtype, "exact")["f32"], cb.exact_reference(s, kernel, with_res)["ref"]
    n, cin, cout, H, W, d = cb.SHAPES[s]
    assert got.shape == (n, cout, H, W)
    bad = got.astype(np.float64) != ref                          # (every value of ref is an fp32 value; -0 == +0)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5].tolist())
    assert (ref > 0).any() and (ref == 0).any()


@pytest.mark.parametrize("s, kernel, with_res, dtype", CASES, ids=IDS)
def test_random_inputs_stay_within_the_bound(s, kernel, with_res, dtype):
    """Measured on the MI355X: the table in DESIGN.md 10w; the limit of 1 stands as derived."""
    got, r = _run(s, kernel, with_res, dtype, "random")["f32"], cb.random_reference(s, kernel, dtype, with_res)
    ratio = np.abs(got.astype(np.float64) - r["ref"]) / r["tol"]
    print("conv_bn %s k%d %s %s: max err / tol %.5f" % (cb.SHAPE_IDS[s], kernel, "res" if with_res else "plain", dtype,
                                                        float(ratio.max())))
    assert ratio.max() <= 1.0, float(ratio.max())
    assert (r["ref"] > 0).any() and (r["ref"] == 0).any()        # ReLU cuts some and not all
    if with_res:                                                  # the residual decides the sign of some
        assert (np.sign(r["pre"]) * np.sign(r["prerelu"]) < 0).any()


@pytest.mark.parametrize("s, kernel, with_res, dtype", RES_CASES, ids=RES_IDS)
def test_without_relu_with_a_residual(s, kernel, with_res, dtype):
    got = _run(s, kernel, True, dtype, "random", relu=False)["f32"]
    r = cb.random_reference(s, kernel, dtype, True, relu=False)
    ratio = np.abs(got.astype(np.float64) - r["ref"]) / r["tol"]
    print("conv_bn %s k%d res %s relu=0: max err / tol %.5f" % (cb.SHAPE_IDS[s], kernel, dtype, float(ratio.max())))
    assert ratio.max() <= 1.0, float(ratio.max())
    assert (got < 0).any()
    e = _run(s, kernel, True, dtype, "exact", relu=False)["f32"]
    assert np.array_equal(e.astype(np.float64), cb.exact_reference(s, kernel, True, relu=False)["ref"])
    assert (e < 0).any()


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("s, kernel, with_res, dtype", CASES, ids=IDS)
def test_half_output_is_the_rne_conversion_of_the_fp32_output(s, kernel, with_res, dtype, kind):
    got = _run(s, kernel, with_res, dtype, kind)
    want = torch.from_numpy(got["f32"]).to(cb.DTYPES[dtype])      # torch's conversion on the CPU: round to nearest even
    assert torch.equal(got["half"].view(torch.int16), want.view(torch.int16))
    if kind == "random":
        assert not torch.equal(want.float(), torch.from_numpy(got["f32"]))   # (the rounding did something)


@pytest.mark.parametrize("s, kernel, with_res, dtype", CASES, ids=IDS)
def test_guards_are_intact(s, kernel, with_res, dtype):
    for kind in ("exact", "random"):
        check_guards(dict(enumerate(_run(s, kernel, with_res, dtype, kind)["guards"])), GUARD, where=kind)


@pytest.mark.parametrize("s, kernel, dtype", [(1, 3, "float16"), (5, 1, "bfloat16"), (7, 3, "bfloat16"), (6, 1, "float16")])
def test_two_runs_give_equal_bytes(s, kernel, dtype):
    first = _run(s, kernel, True, dtype, "random")
    c, x, res, packed = _operands(s, kernel, True, dtype, "random")
    for out_dtype, key in ((torch.float32, "f32"), (None, "half")):
        again = core.conv_bn(x, packed, c["scale"], c["shift"], kernel, cb.dilation_of(s, kernel), residual=res,
                             out_dtype=out_dtype).cpu()
        want = first[key] if key == "half" else torch.from_numpy(first[key])
        assert again.view(torch.uint8).numpy().tobytes() == want.view(torch.uint8).numpy().tobytes()


@pytest.mark.parametrize("kernel", cb.KERNELS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_frame_alone_equals_the_frame_in_a_batch(dtype, kernel):
    s = 2                                                         # a batch of 3
    assert cb.SHAPES[s][0] == 3
    batch = _run(s, kernel, True, dtype, "random")
    c, x, res, packed = _operands(s, kernel, True, dtype, "random")
    for f in (0, 1, 2):
        alone = core.conv_bn(x[f:f + 1].clone(), packed, c["scale"], c["shift"], kernel, cb.dilation_of(s, kernel),
                             residual=res[f:f + 1].clone(), out_dtype=torch.float32)
        assert np.array_equal(alone.cpu().numpy().view(np.uint32)[0], batch["f32"].view(np.uint32)[f])


@pytest.mark.parametrize("s, dtype", [(1, "float16"), (4, "bfloat16"), (5, "bfloat16"), (2, "float16")])
def test_kernel_3_without_residual_gives_f17s_bytes(s, dtype):
    c, x, _, packed = _operands(s, 3, False, dtype, "random")
    old_packed = core.conv3x3_pack_weights(c["w"].copy(), cb.DTYPES[dtype])
    assert torch.equal(packed, old_packed) and packed.numel() == c["w"].size * 2
    d = cb.SHAPES[s][5]
    for out_dtype in (torch.float32, None):
        for relu in (True, False):
            old = core.conv3x3_bn_relu(x, old_packed, c["scale"], c["shift"], d, relu=relu, out_dtype=out_dtype)
            new = core.conv_bn(x, packed, c["scale"], c["shift"], 3, d, relu=relu, out_dtype=out_dtype)
            assert old.dtype == new.dtype and torch.equal(old.view(torch.uint8), new.view(torch.uint8))


@pytest.mark.parametrize("kernel", cb.KERNELS)
@pytest.mark.parametrize("s, dtype", [(2, "float16"), (2, "bfloat16"), (4, "bfloat16")])
def test_the_features_as_residual_equal_the_call_on_a_copy(s, dtype, kernel):
    n, cin, cout, H, W, d = cb.SHAPES[s]
    assert cin == cout
    c, x, _, packed = _operands(s, kernel, False, dtype, "random")
    d = cb.dilation_of(s, kernel)
    same = core.conv_bn(x, packed, c["scale"], c["shift"], kernel, d, residual=x, out_dtype=torch.float32)
    copy = core.conv_bn(x, packed, c["scale"], c["shift"], kernel, d, residual=x.clone(), out_dtype=torch.float32)
    assert torch.equal(same.view(torch.int32), copy.view(torch.int32))
    r = cb.reference(c["x"], c["w"], c["scale"], c["shift"], kernel, d, dtype, residual=c["x"])
    ratio = np.abs(same.cpu().numpy().astype(np.float64) - r["ref"]) / r["tol"]
    assert ratio.max() <= 1.0, float(ratio.max())
    plain = core.conv_bn(x, packed, c["scale"], c["shift"], kernel, d, out_dtype=torch.float32)
    assert not torch.equal(plain, same)


# ---- cnn.ResidualBlock and cnn.DrnDilated ----

def _within_bound(name, dtype, got32, inp, conv, fold, kernel, d, residual=None, relu=True):
    """One launch against the reference evaluated on the device's own inputs of that launch."""
    r = cb.reference(inp.float().cpu().numpy(), conv.weight.detach().numpy(), fold[0].numpy(), fold[1].numpy(), kernel,
                     d, dtype, residual=None if residual is None else residual.float().cpu().numpy(), relu=relu)
    ratio = np.abs(got32.cpu().numpy().astype(np.float64) - r["ref"]) / r["tol"]
    print("conv_bn block %s %s: max err / tol %.5f" % (name, dtype, float(ratio.max())))
    assert ratio.max() <= 1.0, (name, float(ratio.max()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["downsample", "identity", "no_residual"])
def test_residual_block_equals_the_composed_calls(form, dtype):
    td = cb.DTYPES[dtype]
    cin, cout = (32, 64) if form == "downsample" else (32, 32)
    block = Block(cin, cout, dilation=(2, 4), downsample=form == "downsample", residual=form != "no_residual",
                  seed=30).eval()
    x = torch.randn(2, cin, 9, 37, generator=torch.Generator().manual_seed(31)).to(DEV).to(td)
    f1, f2 = cnn.fold_batchnorm(block.bn1), cnn.fold_batchnorm(block.bn2)
    p1, p2 = core.conv_pack_weights(block.conv1.weight, td), core.conv_pack_weights(block.conv2.weight, td)
    y = core.conv_bn(x, p1, *f1, 3, 2)
    res = None
    if form == "downsample":
        fd, pd = cnn.fold_batchnorm(block.downsample[1]), core.conv_pack_weights(block.downsample[0].weight, td)
        res = core.conv_bn(x, pd, *fd, 1, relu=False)
        assert res.dtype == td and (res.float() < 0).any()
        _within_bound("downsample", dtype, core.conv_bn(x, pd, *fd, 1, relu=False, out_dtype=torch.float32), x,
                      block.downsample[0], fd, 1, 1, relu=False)
    elif form == "identity":
        res = x
    want = core.conv_bn(y, p2, *f2, 3, 4, residual=res)
    want32 = core.conv_bn(y, p2, *f2, 3, 4, residual=res, out_dtype=torch.float32)

    rb = cnn.ResidualBlock(block, dtype=td)
    got = rb(x)
    assert got.dtype == td and tuple(got.shape) == (2, cout, 9, 37)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert torch.equal(rb(x, out_dtype=torch.float32).view(torch.int32), want32.view(torch.int32))
    assert len(rb.packed) == (3 if form == "downsample" else 2)
    _within_bound("conv1", dtype, core.conv_bn(x, p1, *f1, 3, 2, out_dtype=torch.float32), x, block.conv1, f1, 3, 2)
    _within_bound("conv2", dtype, want32, y, block.conv2, f2, 3, 4, residual=res)
    if form == "no_residual":    # arch C's layer7 / layer8: f17's launches
        old = core.conv3x3_bn_relu(core.conv3x3_bn_relu(x, p1, *f1, 2), p2, *f2, 4)
        assert torch.equal(got.view(torch.int16), old.view(torch.int16))


def _seq_layer(cin, cout, dilation, seed):
    g = torch.Generator().manual_seed(seed)
    conv = torch.nn.Conv2d(cin, cout, 3, padding=dilation, dilation=dilation, bias=False)
    bn = torch.nn.BatchNorm2d(cout)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / (9 * cout)) ** 0.5)
        bn.running_mean.copy_(torch.randn(cout, generator=g) * 0.2)
        bn.running_var.copy_(torch.rand(cout, generator=g) + 0.5)
        bn.weight.copy_(torch.rand(cout, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(cout, generator=g) * 0.1)
    return torch.nn.Sequential(conv, bn, torch.nn.ReLU()).eval()


@pytest.mark.parametrize("dtype", DTYPES)
def test_drn_dilated_equals_the_composed_calls_and_feeds_the_dp(dtype):
    td = cb.DTYPES[dtype]
    case = helpers.build_case("drn_d_22_unary", 128, 256, 32, seed=3)
    cfg = case["cfg"]
    Hs, Ws, P2S = cfg.rows // 8, cfg.realcols, case["segmentation"].shape[-1]
    assert (Hs, Ws, P2S) == (16, 32, 32) and case["segmentation"].shape[2] == 21
    layer5 = [Block(32, 64, (2, 2), downsample=True, seed=40).eval(), Block(64, 64, (2, 2), seed=44).eval()]
    layer6 = [Block(64, 32, (4, 4), downsample=True, seed=48).eval(), Block(32, 32, (4, 4), seed=52).eval()]
    layer7, layer8 = _seq_layer(32, 64, 2, seed=7), _seq_layer(64, 32, 1, seed=8)
    seg = torch.nn.Conv2d(32, 21, 1, bias=True)
    with torch.no_grad():
        seg.weight.normal_(0, (2.0 / 21) ** 0.5, generator=torch.Generator().manual_seed(9))
        seg.bias.zero_()
    x = torch.randn(1, 32, Hs, Ws, generator=torch.Generator().manual_seed(10)).abs().to(DEV).to(td)

    y = x
    for block in layer5 + layer6:                                 # by hand, launch by launch
        d = block.conv1.dilation[0]
        h = core.conv_bn(y, core.conv_pack_weights(block.conv1.weight, td), *cnn.fold_batchnorm(block.bn1), 3, d)
        res = y if block.downsample is None else core.conv_bn(
            y, core.conv_pack_weights(block.downsample[0].weight, td), *cnn.fold_batchnorm(block.downsample[1]), 1,
            relu=False)
        y = core.conv_bn(h, core.conv_pack_weights(block.conv2.weight, td), *cnn.fold_batchnorm(block.bn2), 3, d,
                         residual=res)
    assert y.dtype == td and tuple(y.shape) == (1, 32, Hs, Ws) and (y > 0).any()
    want_seg, want_cnn = cnn.DrnTail(layer7, layer8, seg, 19, P2S, dtype=td).forward(y, want_cnn_out=True)

    net = cnn.DrnDilated(layer5, layer6, layer7, layer8, seg, 19, P2S, dtype=td)
    assert len(net.blocks) == 4
    got_seg, got_cnn = net.forward(x, want_cnn_out=True)
    assert torch.equal(got_seg, want_seg) and got_seg.dtype == torch.int32 and tuple(got_seg.shape) == (1, Ws, 21, P2S)
    assert torch.equal(got_cnn.view(torch.int32), want_cnn.view(torch.int32))
    assert torch.equal(net(x.float()), want_seg)                  # another floating dtype is converted first

    # the DP takes the network's output: Sections identical to the oracle's on the same int tensor
    case["segmentation"] = got_seg.cpu().numpy()
    ref = helpers.run_oracle(case)
    got = helpers.run_core(case, want_tables=False)
    errs = helpers.compare(ref, got, 0, cfg, check_tables=False)
    assert not errs, errs[:5]
