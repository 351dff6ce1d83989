"""The backbone's stem (f20) on the device against tests/stem_reference.py, pinned as f17-f19 are: inputs whose
arithmetic is exact in both dtypes and in every order must give the float64 reference bit for bit, in `mid` and in
`out`; random inputs must stay within the derived bound (`mid` against the reference from the bytes, `out` against the
reference evaluated on the device's own `mid`), each bound test printing max(err / tol).  Then: `out` without d_mid has
the bytes of `out` with it, guards around both outputs, the image inside a larger allocation of 0xFF bytes (a load
outside the image would change the result; nothing is provoked), determinism, batch invariance, cnn.DrnStem against
core.stem, and cnn.Drn against DrnStem -> DrnDownsampling, launch by launch and in front of the DP."""
import functools

import numpy as np
import pytest
import torch

import helpers
from guards import check_guards
import stem_reference as sr
import test_conv_stride_gpu as f19
from instance_stixels_amd import cnn, core

pytestmark = pytest.mark.gpu

DTYPES = sorted(sr.DTYPES)
CASES = [(s, dt) for s in range(len(sr.SHAPES)) for dt in DTYPES]
IDS = ["%s-%s" % (sr.SHAPE_IDS[s], dt) for s, dt in CASES]
GUARD = 64
DEV = torch.device("cuda", 0)


def _inputs(s, dtype, kind):
    """The case's arrays, with the table of the kind: {0, 1} values (exact) or the reference's normalisation."""
    c = dict(sr.exact_inputs(s) if kind == "exact" else sr.random_inputs(s))
    if kind != "exact":
        c["lut"] = sr.input_table(dtype)
    return c


def _operands(s, dtype, kind):
    c, td = _inputs(s, dtype, kind), sr.DTYPES[dtype]
    image = torch.from_numpy(c["image"].copy()).to(DEV)
    lut = torch.from_numpy(c["lut"].copy()).to(DEV).to(td)
    packed = core.stem_pack_weights(c["w0"].copy(), c["w1"].copy(), td)
    return c, image, lut, packed, (c["scale0"], c["shift0"], c["scale1"], c["shift1"])


@functools.lru_cache(maxsize=None)
def _run(s, dtype, kind):
    """One guarded call with d_mid and one without, on the same device operands."""
    c, image, lut, packed, folds = _operands(s, dtype, kind)
    out, mid, guards = core.stem(image, lut, packed, *folds, want_mid=True, canary=GUARD)
    alone, guards_alone = core.stem(image, lut, packed, *folds, canary=GUARD)
    n, H, W = sr.SHAPES[s]
    for t in (out, mid, alone):
        assert t.dtype == sr.DTYPES[dtype] and tuple(t.shape) == (n, 16, H, W)
    return dict(out=out.cpu(), mid=mid.cpu(), alone=alone.cpu(), guards=[guards["out"], guards["mid"], guards_alone["out"]])


def _bits(t):
    return t.contiguous().view(torch.int16)


def _half(a, dtype):
    return torch.from_numpy(np.asarray(a, np.float32)).to(sr.DTYPES[dtype])


@pytest.mark.parametrize("s, dtype", CASES, ids=IDS)
def test_exact_inputs_give_the_float64_reference_bitwise(s, dtype):
    got, ref = _run(s, dtype, "exact"), sr.exact_reference(s)
    for name in ("mid", "out"):
        want = _half(ref[name], dtype)                 # (every value of ref is an fp32 value; RNE on the CPU)
        bad = _bits(got[name]) != _bits(want)
        # -0 and +0: the reference's max(., 0) gives +0, and so does the device's
        assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad.numpy())[:5].tolist())
    assert torch.equal(got["mid"].double(), torch.from_numpy(ref["mid"].copy()))          # mid itself is exact in the half dtype


@pytest.mark.parametrize("s, dtype", CASES, ids=IDS)
def test_random_inputs_stay_within_the_bound(s, dtype):
    """Measured on the MI355X: the table in DESIGN.md 10z; the limit of 1 stands as derived."""
    got, c = _run(s, dtype, "random"), _inputs(s, dtype, "random")
    rm = sr.random_mid_reference(s, dtype)
    mid = got["mid"].double().numpy()
    ratio_mid = np.abs(mid - rm["ref"]) / rm["tol_half"]
    ro = sr.out_reference(mid, c["w1"], c["scale1"], c["shift1"], dtype)           # on the device's own mid
    ratio_out = np.abs(got["out"].double().numpy() - ro["ref"]) / ro["tol_half"]
    print("stem %s %s: max err / tol  mid %.5f  out %.5f" % (sr.SHAPE_IDS[s], dtype, float(ratio_mid.max()),
                                                            float(ratio_out.max())))
    assert ratio_mid.max() <= 1.0, float(ratio_mid.max())
    assert ratio_out.max() <= 1.0, float(ratio_out.max())
    assert (c["shift0"] > 0.25).sum() * 4 >= c["shift0"].size
    assert (rm["ref"] > 0).any() and (ro["ref"] > 0).any()


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("s, dtype", CASES, ids=IDS)
def test_out_without_mid_has_the_bytes_of_out_with_it(s, dtype, kind):
    got = _run(s, dtype, kind)
    assert torch.equal(_bits(got["alone"]), _bits(got["out"]))


@pytest.mark.parametrize("s, dtype", CASES, ids=IDS)
def test_guards_are_intact(s, dtype):
    for kind in ("exact", "random"):
        check_guards(dict(enumerate(_run(s, dtype, kind)["guards"])), GUARD, where=kind)


@pytest.mark.parametrize("s, dtype", CASES, ids=IDS)
def test_bytes_of_0xff_around_the_image_do_not_change_the_result(s, dtype):
    """The image inside a larger allocation filled with 0xFF on both sides: a load from outside the image would index
    lut[c][255], about +3.8, and change a sum.  The clamped loads of the zero-filled border stay inside."""
    first = _run(s, dtype, "random")
    c, image, lut, packed, folds = _operands(s, dtype, "random")
    margin = max(4096, int(image[0].numel()))
    big = torch.full((image.numel() + 2 * margin,), 0xFF, dtype=torch.uint8, device=DEV)
    inner = big[margin:margin + image.numel()].view(image.shape)
    inner.copy_(image)
    assert inner.is_contiguous() and inner.data_ptr() == big.data_ptr() + margin
    out, mid = core.stem(inner, lut, packed, *folds, want_mid=True)
    assert torch.equal(_bits(out.cpu()), _bits(first["out"])) and torch.equal(_bits(mid.cpu()), _bits(first["mid"]))
    assert torch.equal(inner, image) and int(big[0]) == 0xFF and int(big[-1]) == 0xFF
    assert float(lut[:, 255].float().min()) > 3.0


@pytest.mark.parametrize("s, dtype", CASES, ids=IDS)
def test_two_runs_give_equal_bytes(s, dtype):
    first = _run(s, dtype, "random")
    c, image, lut, packed, folds = _operands(s, dtype, "random")
    out, mid = core.stem(image, lut, packed, *folds, want_mid=True)
    assert torch.equal(_bits(out.cpu()), _bits(first["out"])) and torch.equal(_bits(mid.cpu()), _bits(first["mid"]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s", [i for i, shape in enumerate(sr.SHAPES) if shape[0] > 1])
def test_a_frame_alone_equals_the_frame_in_a_batch(s, dtype):
    batch = _run(s, dtype, "random")
    c, image, lut, packed, folds = _operands(s, dtype, "random")
    for f in range(sr.SHAPES[s][0]):
        out, mid = core.stem(image[f:f + 1].clone(), lut, packed, *folds, want_mid=True)
        assert torch.equal(_bits(out.cpu()[0]), _bits(batch["out"][f]))
        assert torch.equal(_bits(mid.cpu()[0]), _bits(batch["mid"][f]))


# ---- cnn.DrnStem and cnn.Drn ----

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n, rows, cols", [(2, 17, 65), (1, 5, 3)])
def test_drn_stem_gives_the_bytes_of_core_stem(n, rows, cols, dtype):
    td = sr.DTYPES[dtype]
    layer0, layer1 = sr.stem_layers(seed=40)
    image = torch.from_numpy(np.random.default_rng(41).integers(0, 256, (n, rows, cols, 3)).astype(np.uint8)).to(DEV)
    lut = cnn.input_table(sr.MEAN, sr.STD, td).to(DEV)
    packed = core.stem_pack_weights(layer0[0].weight, layer1[0].weight, td)
    folds = cnn.fold_batchnorm(layer0[1]) + cnn.fold_batchnorm(layer1[1])
    want_out, want_mid = core.stem(image, lut, packed, *folds, want_mid=True)
    stem = cnn.DrnStem(layer0, layer1, sr.MEAN, sr.STD, dtype=td)
    assert stem.launches == 1 and torch.equal(stem.packed, packed) and torch.equal(_bits(stem.lut), _bits(lut))
    got_out, got_mid = stem.forward(image, want_mid=True)
    assert got_out.dtype == td and tuple(got_out.shape) == (n, 16, rows, cols)
    assert torch.equal(_bits(got_out), _bits(want_out)) and torch.equal(_bits(got_mid), _bits(want_mid))
    assert torch.equal(_bits(stem(image)), _bits(want_out))
    # ... and within the bound of the modules it was built from
    rm = sr.mid_reference(image.cpu().numpy(), lut.float().cpu().numpy(), layer0[0].weight.detach().numpy(),
                          folds[0].numpy(), folds[1].numpy(), dtype)
    mid = got_mid.double().cpu().numpy()
    ro = sr.out_reference(mid, layer1[0].weight.detach().numpy(), folds[2].numpy(), folds[3].numpy(), dtype)
    ratios = (float((np.abs(mid - rm["ref"]) / rm["tol_half"]).max()),
              float((np.abs(got_out.double().cpu().numpy() - ro["ref"]) / ro["tol_half"]).max()))
    print("stem DrnStem %dx%dx%d %s: max err / tol  mid %.5f  out %.5f" % (n, rows, cols, dtype, *ratios))
    assert max(ratios) <= 1.0, ratios


def _drn(td, p2s):
    layers, seg = f19._model()
    layer0, layer1 = sr.stem_layers(seed=50)
    net = cnn.Drn(layer0, layer1, **layers, seg=seg, n_classes=19, rows_power2_segmentation=p2s, mean=sr.MEAN,
                  std=sr.STD, dtype=td)
    return net, (layer0, layer1), layers, seg


@pytest.mark.parametrize("dtype", DTYPES)
def test_drn_equals_stem_then_downsampling_in_25_launches(dtype, monkeypatch):
    """2 x 37 x 75 x 3 bytes: the bytes of DrnStem followed by DrnDownsampling, the launches counted as they are made,
    and Drn.from_base equal to the explicit constructor."""
    td = sr.DTYPES[dtype]
    net, (layer0, layer1), layers, seg = _drn(td, 8)
    image = torch.from_numpy(np.random.default_rng(51).integers(0, 256, (2, 37, 75, 3)).astype(np.uint8)).to(DEV)
    x = cnn.DrnStem(layer0, layer1, sr.MEAN, sr.STD, dtype=td)(image)
    assert tuple(x.shape) == (2, 16, 37, 75) and x.dtype == td
    want_seg, want_cnn = cnn.DrnDownsampling(**layers, seg=seg, n_classes=19, rows_power2_segmentation=8,
                                             dtype=td).forward(x, want_cnn_out=True)
    assert net.launches == 25
    base = torch.nn.Sequential(layer0, layer1, layers["layer2"], *(torch.nn.Sequential(*layers["layer%d" % i]) for i in (3, 4, 5, 6)),
                               layers["layer7"], layers["layer8"])
    assert len(base) == 9
    other = cnn.Drn.from_base(base, seg, 19, 8, sr.MEAN, sr.STD, dtype=td)
    assert other.launches == 25
    launches = []
    for name in ("stem", "conv_bn_stride", "conv_bn", "conv3x3_bn_relu", "segmentation_head"):
        def counted(*args, _fn=getattr(core, name), _name=name, **kwargs):
            launches.append(_name)
            return _fn(*args, **kwargs)
        monkeypatch.setattr(core, name, counted)
    got_seg, got_cnn = net.forward(image, want_cnn_out=True)
    assert launches == ["stem"] + ["conv_bn_stride"] * 23 + ["segmentation_head"]
    assert tuple(got_cnn.shape) == (2, 21, 5, 10) and tuple(got_seg.shape) == (2, 10, 21, 8)
    assert torch.equal(got_seg, want_seg) and torch.equal(got_cnn.view(torch.int32), want_cnn.view(torch.int32))
    seg2, cnn2 = other(image, want_cnn_out=True)
    assert torch.equal(seg2, want_seg) and torch.equal(cnn2.view(torch.int32), want_cnn.view(torch.int32))


@pytest.mark.parametrize("dtype", DTYPES)
def test_drn_feeds_the_dp(dtype):
    """The network's output from a 128 x 256 image as the DP's input: Sections identical to the oracle's on the same
    int tensor."""
    td = sr.DTYPES[dtype]
    case = helpers.build_case("drn_d_22_unary", 128, 256, 32, seed=3)
    cfg = case["cfg"]
    Ws, P2S = cfg.realcols, case["segmentation"].shape[-1]
    assert (cfg.rows // 8, Ws, P2S) == (16, 32, 32) and case["segmentation"].shape[2] == 21
    net, _, _, _ = _drn(td, P2S)
    image = torch.from_numpy(np.random.default_rng(52).integers(0, 256, (1, 128, 256, 3)).astype(np.uint8)).to(DEV)
    got_seg = net(image)
    assert got_seg.dtype == torch.int32 and tuple(got_seg.shape) == (1, Ws, 21, P2S)
    case["segmentation"] = got_seg.cpu().numpy()
    ref = helpers.run_oracle(case)
    got = helpers.run_core(case, want_tables=False)
    errs = helpers.compare(ref, got, 0, cfg, check_tables=False)
    assert not errs, errs[:5]
