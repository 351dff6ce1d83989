"""The segmentation head (f13) on the device against tests/head_reference.py: the k-order pin on the regression
channels (bitwise), the class channels within the contract's bound, the int tensor as FlipAndPad of the call's own
float output (bitwise, two-stage: no int is compared against a float64 reference), guards, dtypes, batch invariance
and the host class in front of ComputeBatch."""
import functools

import numpy as np
import pytest

from guards import check_guards
import head_reference as hr
import helpers
from instance_stixels_amd import core, host

pytestmark = pytest.mark.gpu

# (n, K, rows8, cols8, P2S)
SHAPES = [
    (1, 8, 5, 7, 8),          # smaller than any tile
    (3, 24, 7, 33, 8),        # one pad row, a ragged column tile, K that is not a multiple of 16
    (2, 512, 16, 40, 32),     # the real K, 16 pad rows
    (1, 512, 98, 224, 128),   # the reference's own operating point
    (2, 64, 128, 256, 256),   # C3's plane
]
# (n_classes, n_regression, clamp)
SPLITS = [(19, 2, None), (19, 3, (19, 0.0, 128.0)), (19, 0, None), (30, 2, None)]
CASES = [(s, 0) for s in range(len(SHAPES))] + [(1, k) for k in range(1, len(SPLITS))]
IDS = ["%dx%dx%dx%d-p%d-%d+%d" % (SHAPES[s] + SPLITS[k][:2]) for s, k in CASES]
GUARD = 64
DOMINANT = (1, 2)   # (shape, frame): class 3 raised by 40 there


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _inputs(s, k):
    """The issue's random inputs of a case and its reference, computed once and left unchanged."""
    n, K, Hs, Ws, P2S = SHAPES[s]
    ncls, nreg, clamp = SPLITS[k]
    x, w, b = hr.random_inputs(n, K, Hs, Ws, ncls + nreg, seed=100 * s + k)
    if s == DOMINANT[0]:
        # feature 0 is 1 in one frame and 0 in the others, and only class 3 weighs it: that frame's class-3 logits
        # are 40 above the rest, its y[3] is 1e-17 to 1e-14 (often 0 in the contract's binary64) and its other y about 40
        x[:, 0] = 0.0
        x[DOMINANT[1], 0] = 1.0
        w[:, 0] = 0.0
        w[3, 0] = 40.0
    z = hr.logits(x, w, b)
    ref = hr.cnn_out(z, ncls, clamp)
    for a in (x, w, b, z, ref):
        a.setflags(write=False)
    return dict(x=x, w=w, b=b, z=z, ref=ref, ncls=ncls, clamp=clamp, P2S=P2S)


@functools.lru_cache(maxsize=None)
def _run(s, k):
    """One guarded call with both outputs."""
    torch, dev = _torch()
    c = _inputs(s, k)
    seg, cnn, guards = core.segmentation_head(torch.tensor(c["x"], device=dev), c["w"], c["b"], c["ncls"], c["P2S"],
                                              want_cnn_out=True, clamp=c["clamp"], canary=GUARD)
    return dict(seg=seg.cpu().numpy(), cnn=cnn.cpu().numpy(), guards=guards)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("s, k", CASES, ids=IDS)
def test_regression_channels_are_the_fmaf_chain_bitwise(s, k):
    c, got = _inputs(s, k), _run(s, k)
    ncls = c["ncls"]
    if c["ref"].shape[1] == ncls:
        assert got["cnn"].shape[1] == ncls
        return
    assert np.array_equal(_bits(got["cnn"][:, ncls:]), _bits(c["ref"][:, ncls:]))
    if c["clamp"] is not None:
        ch, lo, hi = c["clamp"]
        assert (c["z"][:, ch] < lo).any()       # the clamp does something in this case
        assert got["cnn"][:, ch].min() >= lo and got["cnn"][:, ch].max() <= hi


@pytest.mark.parametrize("s, k", CASES, ids=IDS)
def test_class_channels_within_the_bound(s, k):
    c, got = _inputs(s, k), _run(s, k)
    ncls = c["ncls"]
    ref64 = hr.class_values64(c["z"], ncls)
    err = np.abs(got["cnn"][:, :ncls].astype(np.float64) - ref64)
    tol = hr.class_tolerance(c["z"], ncls)
    print("class channels: max err / tol", float((err / tol).max()), "max err", float(err.max()))
    assert (err <= tol).all(), float((err / tol).max())
    if s == DOMINANT[0]:
        f = DOMINANT[1]
        assert (ref64[f, 3] < 1e-12).all() and (ref64[f, 0] > 30).all()
        assert (got["cnn"][f, 3] < 1e-10).all() and (got["cnn"][f, 0] > 30).all()


@pytest.mark.parametrize("s, k", CASES, ids=IDS)
def test_int_tensor_is_flip_and_pad_of_the_float_output(s, k):
    torch, dev = _torch()
    c, got = _inputs(s, k), _run(s, k)
    n, K, Hs, Ws, P2S = SHAPES[s]
    assert got["seg"].shape == (n, Ws, c["ref"].shape[1], P2S) and got["seg"].dtype == np.int32
    assert np.array_equal(got["seg"], hr.segmentation(got["cnn"], P2S))
    assert not got["seg"][..., Hs:].any()                                   # every pad row is zero
    assert np.array_equal(got["seg"], core.flip_and_pad(got["cnn"], P2S))   # ... and the device's own FlipAndPad
    x = torch.tensor(c["x"], device=dev)
    only_seg = core.segmentation_head(x, c["w"], c["b"], c["ncls"], P2S, clamp=c["clamp"])
    only_cnn = core.segmentation_head(x, c["w"], c["b"], c["ncls"], P2S, clamp=c["clamp"], want_segmentation=False)
    assert np.array_equal(only_seg.cpu().numpy(), got["seg"])
    assert np.array_equal(_bits(only_cnn.cpu().numpy()), _bits(got["cnn"]))


@pytest.mark.parametrize("s, k", CASES, ids=IDS)
def test_guards_are_intact(s, k):
    check_guards(_run(s, k)["guards"], GUARD, {"segmentation", "cnn_out"})


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_half_features_equal_the_widened_fp32_call(dtype):
    torch, dev = _torch()
    c = _inputs(2, 0)
    xh = torch.tensor(c["x"], device=dev).to(getattr(torch, dtype))
    wide = xh.to(torch.float32)
    assert not torch.equal(wide, torch.tensor(c["x"], device=dev))          # (the rounding to half did something)
    seg_h, cnn_h = core.segmentation_head(xh, c["w"], c["b"], c["ncls"], c["P2S"], want_cnn_out=True)
    seg_w, cnn_w = core.segmentation_head(wide, c["w"], c["b"], c["ncls"], c["P2S"], want_cnn_out=True)
    assert np.array_equal(_bits(cnn_h.cpu().numpy()), _bits(cnn_w.cpu().numpy()))
    assert np.array_equal(seg_h.cpu().numpy(), seg_w.cpu().numpy())
    # and the widened call is the reference's chain on those values
    z = hr.logits(wide.cpu().numpy(), c["w"], c["b"])
    assert np.array_equal(_bits(cnn_w.cpu().numpy()[:, c["ncls"]:]), _bits(z[:, c["ncls"]:]))


def test_batch_invariance_and_determinism():
    torch, dev = _torch()
    c, got = _inputs(1, 0), _run(1, 0)
    x = torch.tensor(c["x"], device=dev)
    seg1, cnn1 = core.segmentation_head(x[1:2], c["w"], c["b"], c["ncls"], c["P2S"], want_cnn_out=True)
    assert np.array_equal(seg1.cpu().numpy()[0], got["seg"][1])
    assert np.array_equal(_bits(cnn1.cpu().numpy()[0]), _bits(got["cnn"][1]))
    seg2, cnn2 = core.segmentation_head(x, c["w"], c["b"], c["ncls"], c["P2S"], want_cnn_out=True)
    assert seg2.cpu().numpy().tobytes() == got["seg"].tobytes()
    assert cnn2.cpu().numpy().tobytes() == got["cnn"].tobytes()


HOST_SEED = 0   # chosen so that the reference's int tensor equals the device's (asserted first below)


def test_host_class_feeds_compute_batch():
    """SetSegmentationHead, SegmentationHeadBatch, ComputeBatch on its output: the Sections of ComputeBatch on
    oracle.flip_and_pad(reference float output), bitwise."""
    torch, dev = _torch()
    n, K = 2, 64
    case = helpers.build_case("drn_d_22_unary", 128, 256, 32, seed=3, n_images=n)
    cfg = case["cfg"]
    Hs, Ws, P2S = cfg.rows // 8, cfg.realcols, case["segmentation"].shape[-1]
    assert (Hs, Ws, P2S) == (16, 32, 32) and case["segmentation"].shape[2] == 21
    x, w, b = hr.random_inputs(n, K, Hs, Ws, 21, seed=HOST_SEED)
    ref_cnn = hr.cnn_out(hr.logits(x, w, b), 19)
    ref_seg = hr.segmentation(ref_cnn, P2S)
    st = host.Stixels()
    st.SetConfig(cfg)
    st.Initialize(max_batch=n)
    with pytest.raises(ValueError, match="SetSegmentationHead"):
        st.SegmentationHeadBatch(n, 0x1000, core.HEAD_F32, 0x2000)
    st.SetSegmentationHead(w, b, K)
    d_x = torch.from_numpy(x).to(dev)
    d_seg = torch.full((n, Ws, 21, P2S), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    d_cnn = torch.empty((n, 21, Hs, Ws), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    st.SegmentationHeadBatch(n, d_x.data_ptr(), core.HEAD_F32, d_seg.data_ptr(), d_cnn.data_ptr(), stream)
    torch.cuda.synchronize()
    assert st.LastFrames() == 0                                               # a producer, not a compute call
    assert np.array_equal(d_seg.cpu().numpy(), ref_seg), "the head's int tensor differs from the reference's"
    with pytest.raises(ValueError, match="n_images"):
        st.SegmentationHeadBatch(n + 1, d_x.data_ptr(), core.HEAD_F32, d_seg.data_ptr())
    with pytest.raises(ValueError, match="dtype"):
        st.SegmentationHeadBatch(n, d_x.data_ptr(), 7, d_seg.data_ptr())
    big = torch.from_numpy(case["disparity"]).to(dev)
    road = [(f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground) for f in case["frames"]]
    got, _ = st.ComputeBatch(cfg.pairwise, big.data_ptr(), d_seg.data_ptr(), road, with_instances=False)
    d_ref = torch.from_numpy(ref_seg).to(dev)
    want, _ = st.ComputeBatch(cfg.pairwise, big.data_ptr(), d_ref.data_ptr(), road, with_instances=False)
    for i in range(n):
        assert helpers.sections_equal(want[i].sections, got[i].sections), f"frame {i}"
    st.close()
