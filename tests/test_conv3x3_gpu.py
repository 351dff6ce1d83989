"""The backbone tail (f17) on the device against tests/conv3x3_reference.py.  The summation inside one MFMA is not
specified, so the kernel is pinned two ways: inputs whose arithmetic is exact in every order must give the float64
reference bit for bit (any wrong, missing or doubled term at every shape), and random inputs must stay within the
derived bound tol = |scale| 9 channels_in 2^-23 sum|w x| + ulp_fp32(ref); each bound test prints max(err / tol).
Then: the half output as the RNE conversion of the same call's fp32 output, relu = 0, guards, determinism, batch
invariance, and the three-launch chain layer7 -> layer8 -> head against cnn.DrnTail and in front of the DP."""
import functools

import numpy as np
import pytest
import torch

import conv3x3_reference as cr
from guards import check_guards
import helpers
from instance_stixels_amd import cnn, core

pytestmark = pytest.mark.gpu

DTYPES = sorted(cr.DTYPES)
CASES = [(s, dt) for s in range(len(cr.SHAPES)) for dt in DTYPES]
IDS = ["%s-%s" % (cr.SHAPE_IDS[s], dt) for s, dt in CASES]
GUARD = 64
DEV = torch.device("cuda", 0)


def _inputs(s, kind):
    return cr.exact_inputs(s) if kind == "exact" else cr.random_inputs(s)


@functools.lru_cache(maxsize=None)
def _run(s, dtype, kind, relu=True):
    """One guarded call with fp32 output and one with half output, on the same device operands."""
    c, td = _inputs(s, kind), cr.DTYPES[dtype]
    x = torch.from_numpy(c["x"].copy()).to(DEV).to(td)
    packed = core.conv3x3_pack_weights(c["w"].copy(), td)
    d = cr.SHAPES[s][5]
    f32, g32 = core.conv3x3_bn_relu(x, packed, c["scale"], c["shift"], d, relu=relu, out_dtype=torch.float32,
                                    canary=GUARD)
    half, g16 = core.conv3x3_bn_relu(x, packed, c["scale"], c["shift"], d, relu=relu, canary=GUARD)
    assert half.dtype == td and f32.dtype == torch.float32
    return dict(f32=f32.cpu().numpy(), half=half.cpu(), guards=(g32["out"], g16["out"]))


@pytest.mark.parametrize("s, dtype", CASES, ids=IDS)
def test_exact_inputs_give_the_float64_reference_bitwise(s, dtype):
    got, ref = _run(s, dtype, "exact")["f32"], cr.exact_reference(s)["ref"]
    n, cin, cout, H, W, d = cr.SHAPES[s]
    assert got.shape == (n, cout, H, W)
    bad = got.astype(np.float64) != ref                          # (every value of ref is an fp32 value; -0 == +0)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5].tolist())
    assert (ref > 0).any()


@pytest.mark.parametrize("s, dtype", CASES, ids=IDS)
def test_random_inputs_stay_within_the_bound(s, dtype):
    """Measured on the MI355X: max(err / tol) between 0.0002 (K = 4608) and 0.0034 over the shapes and both dtypes
    (the table in DESIGN.md 10u); the limit of 1 stands as derived."""
    got, r = _run(s, dtype, "random")["f32"], cr.random_reference(s, dtype)
    ratio = np.abs(got.astype(np.float64) - r["ref"]) / r["tol"]
    print("conv3x3 %s %s: max err / tol %.5f" % (cr.SHAPE_IDS[s], dtype, float(ratio.max())))
    assert ratio.max() <= 1.0, float(ratio.max())
    assert (r["ref"] > 0).any() and (r["ref"] == 0).any()        # ReLU cuts some and not all


@pytest.mark.parametrize("s, dtype", CASES, ids=IDS)
def test_without_relu(s, dtype):
    got, r = _run(s, dtype, "random", relu=False)["f32"], cr.random_reference(s, dtype, relu=False)
    ratio = np.abs(got.astype(np.float64) - r["ref"]) / r["tol"]
    print("conv3x3 %s %s relu=0: max err / tol %.5f" % (cr.SHAPE_IDS[s], dtype, float(ratio.max())))
    assert ratio.max() <= 1.0, float(ratio.max())
    assert (got < 0).any()
    if s < 4:
        e = _run(s, dtype, "exact", relu=False)["f32"]
        assert np.array_equal(e.astype(np.float64), cr.exact_reference(s, relu=False)["ref"])
        assert (e < 0).any()


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("s, dtype", CASES, ids=IDS)
def test_half_output_is_the_rne_conversion_of_the_fp32_output(s, dtype, kind):
    got = _run(s, dtype, kind)
    want = torch.from_numpy(got["f32"]).to(cr.DTYPES[dtype])      # torch's conversion on the CPU: round to nearest even
    assert torch.equal(got["half"].view(torch.int16), want.view(torch.int16))
    if kind == "random":
        assert not torch.equal(want.float(), torch.from_numpy(got["f32"]))   # (the rounding did something)


@pytest.mark.parametrize("s, dtype", CASES, ids=IDS)
def test_guards_are_intact(s, dtype):
    for kind in ("exact", "random"):
        check_guards(dict(enumerate(_run(s, dtype, kind)["guards"])), GUARD, where=kind)


@pytest.mark.parametrize("s, dtype", [(1, "float16"), (4, "bfloat16")])
def test_two_runs_give_equal_bytes(s, dtype):
    c, td, first = cr.random_inputs(s), cr.DTYPES[dtype], _run(s, dtype, "random")
    x = torch.from_numpy(c["x"].copy()).to(DEV).to(td)
    packed = core.conv3x3_pack_weights(c["w"].copy(), td)
    for out_dtype, key in ((torch.float32, "f32"), (None, "half")):
        again = core.conv3x3_bn_relu(x, packed, c["scale"], c["shift"], cr.SHAPES[s][5], out_dtype=out_dtype).cpu()
        want = first[key] if key == "half" else torch.from_numpy(first[key])
        assert again.view(torch.uint8).numpy().tobytes() == want.view(torch.uint8).numpy().tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_frame_alone_equals_the_frame_in_a_batch(dtype):
    s = 2                                                         # a batch of 3
    assert cr.SHAPES[s][0] == 3
    c, td, batch = cr.random_inputs(s), cr.DTYPES[dtype], _run(s, dtype, "random")
    packed = core.conv3x3_pack_weights(c["w"].copy(), td)
    for f in (0, 1, 2):
        x = torch.from_numpy(c["x"][f:f + 1].copy()).to(DEV).to(td)
        alone = core.conv3x3_bn_relu(x, packed, c["scale"], c["shift"], cr.SHAPES[s][5], out_dtype=torch.float32)
        assert np.array_equal(alone.cpu().numpy().view(np.uint32)[0], batch["f32"].view(np.uint32)[f])


# ---- layer7 -> layer8 -> head ----

def _layer(cin, cout, dilation, seed):
    """One layer as the reference's _make_conv_layers builds and initialises it (drn.py:223-233, :191-194), with
    BatchNorm statistics as after training."""
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
def test_three_launch_chain_equals_drn_tail_and_feeds_the_dp(dtype):
    td = cr.DTYPES[dtype]
    case = helpers.build_case("drn_d_22_unary", 128, 256, 32, seed=3)
    cfg = case["cfg"]
    Hs, Ws, P2S = cfg.rows // 8, cfg.realcols, case["segmentation"].shape[-1]
    assert (Hs, Ws, P2S) == (16, 32, 32) and case["segmentation"].shape[2] == 21
    layer7, layer8 = _layer(32, 64, 2, seed=7), _layer(64, 32, 1, seed=8)
    seg = torch.nn.Conv2d(32, 21, 1, bias=True)
    with torch.no_grad():
        seg.weight.normal_(0, (2.0 / 21) ** 0.5, generator=torch.Generator().manual_seed(9))
        seg.bias.zero_()
    x = torch.randn(1, 32, Hs, Ws, generator=torch.Generator().manual_seed(10)).abs().to(DEV).to(td)

    # by hand: two calls of the convolution, the second fed the first's half output, then the head
    folds = [cnn.fold_batchnorm(l[1]) for l in (layer7, layer8)]
    packs = [core.conv3x3_pack_weights(l[0].weight, td) for l in (layer7, layer8)]
    y7 = core.conv3x3_bn_relu(x, packs[0], *folds[0], 2)
    y8 = core.conv3x3_bn_relu(y7, packs[1], *folds[1], 1)
    assert y7.dtype == td and y8.dtype == td
    want_seg, want_cnn = core.segmentation_head(y8, seg.weight, seg.bias, 19, P2S, want_cnn_out=True)

    tail = cnn.DrnTail(layer7, layer8, seg, 19, P2S, dtype=td)
    got_seg, got_cnn = tail.forward(x, want_cnn_out=True)
    assert torch.equal(got_seg, want_seg) and got_seg.dtype == torch.int32 and tuple(got_seg.shape) == (1, Ws, 21, P2S)
    assert torch.equal(got_cnn.view(torch.int32), want_cnn.view(torch.int32))
    assert torch.equal(tail(x.float()), want_seg)                 # another floating dtype is converted first

    # each layer within the bound, the second against the reference on the device's own first-layer output
    for name, inp, layer, fold, pack, d in (("layer7", x, layer7, folds[0], packs[0], 2),
                                            ("layer8", y7, layer8, folds[1], packs[1], 1)):
        f32 = core.conv3x3_bn_relu(inp, pack, *fold, d, out_dtype=torch.float32).cpu().numpy()
        r = cr.reference(inp.float().cpu().numpy(), layer[0].weight.detach().numpy(), fold[0].numpy(), fold[1].numpy(),
                         d, dtype)
        ratio = np.abs(f32.astype(np.float64) - r["ref"]) / r["tol"]
        print("conv3x3 chain %s %s: max err / tol %.5f" % (name, dtype, float(ratio.max())))
        assert ratio.max() <= 1.0, (name, float(ratio.max()))

    # the DP takes the tail's output: Sections identical to the oracle's on the same int tensor
    case["segmentation"] = got_seg.cpu().numpy()
    ref = helpers.run_oracle(case)
    got = helpers.run_core(case, want_tables=False)
    errs = helpers.compare(ref, got, 0, cfg, check_tables=False)
    assert not errs, errs[:5]

    with pytest.raises(core.CoreError, match="eval"):
        cnn.DrnTail(layer7.train(), layer8, seg, 19, P2S, dtype=td)
