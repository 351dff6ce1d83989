"""The CNN label maps (f15) on the device, bitwise against tests/cnn_labels_reference.py throughout: the cell classes,
the label image and the confusion table in both modes, margins, channel and class counts, a caller's table, every
choice of optional outputs, guards, hostile planes (ties, NaN, +inf in border cells), batch invariance, determinism,
the head's own output as the input, the host class and evaluation.cnn_scores."""
import functools

import numpy as np
import pytest

import cnn_labels_reference as cr
import head_reference as hr
import helpers
from guards import check_guards
from instance_stixels_amd import core, evaluation, host

pytestmark = pytest.mark.gpu

# (n, rows8, cols8)
SHAPES = [
    (1, 1, 1),        # one cell: every pixel has missing taps
    (1, 2, 3),
    (3, 5, 7),
    (2, 13, 33),      # ragged tiles in both directions
    (1, 98, 224),     # the reference's operating point
    (1, 128, 256),    # C3's plane
]
MODES = ["nearest", "deconv"]
GUARD = 64
NL = 34


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _gt(n, rows, cols, seed):
    """Ground truth with every labelId, and values >= n_labels (255 and 34 .. 40) that must not be counted."""
    rng = np.random.default_rng(seed)
    gt = rng.integers(0, NL + 7, (n, rows, cols)).astype(np.uint8)
    gt[rng.random(gt.shape) < 0.05] = 255
    return gt


def _guarded_table(start):
    """A device int64 table holding `start` between guard elements: (the whole allocation, the table's view)."""
    torch, dev = _torch()
    nl = start.shape[0]
    full = torch.full((nl * nl + 2 * GUARD,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    full[GUARD: GUARD + nl * nl] = torch.tensor(start.astype(np.int64).ravel(), device=dev)
    return full, full[GUARD: GUARD + nl * nl].view(nl, nl)


def _call(x, n_classes, mode, gt=None, start=None, n_labels=NL, **kw):
    """One guarded call with every output; the table is added to `start`.  Returns numpy copies."""
    torch, dev = _torch()
    full = conf = None
    if gt is not None:
        full, conf = _guarded_table(np.zeros((n_labels, n_labels), np.uint64) if start is None else start)
    out = core.cnn_label_maps(torch.tensor(x, device=dev), n_classes, mode=mode,
                              gt_label=None if gt is None else torch.tensor(gt, device=dev), n_labels=n_labels,
                              confusion=conf, want_class8=True, canary=GUARD, **kw)
    check_guards(out["guards"], GUARD, ("label", "class8"))
    got = dict(label=out["label"].cpu().numpy(), class8=out["class8"].cpu().numpy())
    if gt is not None:
        h = full.cpu().numpy()
        assert (h[:GUARD] == 0x5A5A5A5A5A5A5A5A).all() and (h[-GUARD:] == 0x5A5A5A5A5A5A5A5A).all()
        got["confusion"] = h[GUARD:-GUARD].reshape(n_labels, n_labels).astype(np.uint64)
    return got


def _expect(x, n_classes, mode, gt=None, start=None, n_labels=NL, cols=None, class_to_label=None):
    c8, label = cr.label_maps(x, n_classes, mode, cols=cols, class_to_label=class_to_label)
    want = dict(label=label, class8=c8)
    if gt is not None:
        want["confusion"] = cr.confusion(label, gt, n_labels, 8 * x.shape[3], start)
    return want


def _assert_equal(got, want):
    assert set(got) == set(want)
    for name in want:
        assert got[name].shape == want[name].shape and got[name].dtype == want[name].dtype, name
        bad = int((got[name] != want[name]).sum())
        assert bad == 0, f"{name}: {bad} of {want[name].size} elements differ"


@functools.lru_cache(maxsize=None)
def _case(s):
    """The random planes, ground truth and non-zero starting table of a shape, made once and left unchanged."""
    n, Hs, Ws = SHAPES[s]
    x = cr.random_costs(n, 21, Hs, Ws, seed=50 + s)
    gt = _gt(n, 8 * Hs, 8 * Ws, seed=70 + s)
    start = np.random.default_rng(90 + s).integers(0, 1 << 40, (NL, NL)).astype(np.uint64)
    for a in (x, gt, start):
        a.setflags(write=False)
    return x, gt, start


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("s", range(len(SHAPES)), ids=["%dx%dx%d" % t for t in SHAPES])
def test_outputs_are_the_reference_bitwise(s, mode):
    x, gt, start = _case(s)
    got = _call(x, 19, mode, gt, start)
    want = _expect(x, 19, mode, gt, start)
    _assert_equal(got, want)
    assert (want["confusion"] != start).any() and want["confusion"].sum() < start.sum() + gt.size  # (some gt skipped)
    if mode == "deconv" and s >= 2:
        near = cr.label_maps(x, 19, "nearest")[1]
        assert (near != want["label"]).any()                                 # (the two modes are not the same image)


@pytest.mark.parametrize("mode", MODES)
def test_margin_pixels_are_zero_and_not_scored(mode):
    x, _, start = _case(2)
    n, Hs, Ws = SHAPES[2]
    cols = 8 * Ws + 13
    gt = _gt(n, 8 * Hs, cols, seed=3)
    got = _call(x, 19, mode, gt, start, cols=cols)
    assert got["label"].shape == (n, 8 * Hs, cols) and not got["label"][:, :, 8 * Ws:].any()
    _assert_equal(got, _expect(x, 19, mode, gt, start, cols=cols))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("channels, n_classes", [(21, 19), (22, 19), (21, 1), (32, 32), (40, 32)])
def test_channel_and_class_counts(channels, n_classes, mode):
    n, Hs, Ws = SHAPES[2]
    x = cr.random_costs(n, channels, Hs, Ws, seed=channels + n_classes, n_classes=n_classes)
    gt = _gt(n, 8 * Hs, 8 * Ws, seed=4)
    got = _call(x, n_classes, mode, gt)
    _assert_equal(got, _expect(x, n_classes, mode, gt))
    if n_classes == 32:
        assert (got["class8"] >= 19).any() and (got["label"] == 0).any()     # classes outside the default table: 0
    if n_classes == 1:
        assert not got["class8"].any() and (got["label"] == 7).all()


@pytest.mark.parametrize("mode", MODES)
def test_callers_table_with_a_class_beyond_n_labels(mode):
    x, gt, start = _case(2)
    table = np.arange(19, dtype=np.uint8) + 1
    table[3], table[11] = 200, 20                                            # both >= n_labels = 20: never counted
    nl = 20
    start = np.ascontiguousarray(start[:nl, :nl])
    got = _call(x, 19, mode, gt, start, n_labels=nl, class_to_label=table)
    want = _expect(x, 19, mode, gt, start, n_labels=nl, class_to_label=table)
    _assert_equal(got, want)
    assert (want["label"] == 200).any() and (want["label"] == 20).any()


@pytest.mark.parametrize("mode", MODES)
def test_every_choice_of_outputs_gives_the_same_bytes(mode):
    torch, dev = _torch()
    x, gt, start = _case(3)
    want = _expect(x, 19, mode, gt, start)
    d_x, d_gt = torch.tensor(x, device=dev), torch.tensor(gt, device=dev)
    for label in (False, True):
        for class8 in (False, True):
            for conf in (False, True):
                if not (label or class8 or conf):
                    with pytest.raises(core.CoreError):
                        core.cnn_label_maps(d_x, 19, mode=mode, want_label=False)
                    continue
                full = table = None
                if conf:
                    full, table = _guarded_table(start)
                out = core.cnn_label_maps(d_x, 19, mode=mode, gt_label=d_gt if conf else None, confusion=table,
                                          want_label=label, want_class8=class8, canary=GUARD)
                names = [k for k, v in (("label", label), ("class8", class8)) if v]
                check_guards(out["guards"], GUARD, names)
                assert set(out) == set(names) | {"guards"} | ({"confusion"} if conf else set())
                for k in names:
                    assert np.array_equal(out[k].cpu().numpy(), want[k]), (k, label, class8, conf)
                if conf:
                    h = full.cpu().numpy()
                    assert (h[:GUARD] == h[0]).all() and (h[-GUARD:] == h[0]).all() and h[0] == 0x5A5A5A5A5A5A5A5A
                    assert np.array_equal(h[GUARD:-GUARD].reshape(NL, NL).astype(np.uint64), want["confusion"])


def _hostile():
    """Planes [4][19][5][7] built to break an arg-min: see the asserts of the test."""
    rng = np.random.default_rng(8)
    x = cr.random_costs(4, 19, 5, 7, seed=9)
    x[0, 4] = np.minimum(x[0, 4], 0.25)                                      # often the minimum ...
    x[0, 12] = x[0, 4]                                                       # ... of two equal planes: the lower wins
    x[1] = (rng.integers(0, 4, x[1].shape) / 4.0).astype(np.float32)         # quantised: many exact ties
    x[2, 5] = np.nan                                                         # a NaN plane
    x[2, :, 2, 3] = np.nan                                                   # an all-NaN cell
    x[2, 0, 4, 1] = np.nan                                                   # NaN in class 0: never replaced
    x[3, 6, 0, 0] = np.inf                                                   # +inf in a corner cell ...
    x[3, 6, 4, 6] = np.inf
    x[3, 6, 0, 3] = np.inf                                                   # ... and in edge cells of one class
    x[3, 6, 2, 0] = np.inf
    x[3, 6, 4, 2] = np.inf
    x[3, 6, 3, 6] = np.inf
    x[3, 9, 2, 2] = -np.inf                                                  # -inf next to +inf taps of another class
    return x


@pytest.mark.parametrize("mode", MODES)
def test_hostile_planes(mode):
    x = _hostile()
    gt = _gt(4, 40, 56, seed=10)
    got = _call(x, 19, mode, gt)
    want = _expect(x, 19, mode, gt)
    _assert_equal(got, want)
    table = cr.CITYSCAPES
    assert (want["label"][0] == table[4]).any() and not (want["label"][0] == table[12]).any()
    assert want["class8"][2, 2, 3] == 0 and want["class8"][2, 4, 1] == 0
    assert not (want["label"][2] == table[5]).any()
    if mode == "deconv":
        _, _, up = cr.classes(x, 19, mode, want_values=True)
        assert not np.isnan(up[3]).any() and np.isinf(up[3, 6, :4, :4]).all()  # skipped taps: inf, never NaN
        exact_ties = np.sort(up[1], axis=0)
        assert (exact_ties[0] == exact_ties[1]).mean() > 0.01


@pytest.mark.parametrize("mode", MODES)
def test_batch_invariance_and_determinism(mode):
    x, gt, start = _case(2)
    whole = _call(x, 19, mode, gt, start)
    again = _call(x, 19, mode, gt, start)
    for k in whole:
        assert whole[k].tobytes() == again[k].tobytes(), k
    total = np.zeros((NL, NL), np.uint64)
    for i in range(x.shape[0]):
        alone = _call(np.ascontiguousarray(x[i:i + 1]), 19, mode, np.ascontiguousarray(gt[i:i + 1]))
        assert np.array_equal(alone["label"][0], whole["label"][i])
        assert np.array_equal(alone["class8"][0], whole["class8"][i])
        total += alone["confusion"]
    assert np.array_equal(total + start, whole["confusion"])


@pytest.mark.parametrize("mode", MODES)
def test_two_stage_with_the_heads_own_output(mode):
    """core.segmentation_head on random features, then core.cnn_label_maps on the device's own float output: equal to
    the reference on those bytes."""
    torch, dev = _torch()
    n, K, Hs, Ws = 2, 64, 13, 33
    f, w, b = hr.random_inputs(n, K, Hs, Ws, 21, seed=21)
    cnn = core.segmentation_head(torch.from_numpy(f).to(dev), w, b, 19, 16, want_segmentation=False)
    x = cnn.cpu().numpy()
    gt = _gt(n, 8 * Hs, 8 * Ws, seed=22)
    out = core.cnn_label_maps(cnn, 19, mode=mode, gt_label=torch.from_numpy(gt).to(dev), want_class8=True)
    got = dict(label=out["label"].cpu().numpy(), class8=out["class8"].cpu().numpy(),
               confusion=out["confusion"].cpu().numpy().astype(np.uint64))
    _assert_equal(got, _expect(x, 19, mode, gt))
    assert len(np.unique(got["class8"])) > 3


@pytest.mark.parametrize("mode", MODES)
def test_host_class_equals_the_direct_call(mode):
    torch, dev = _torch()
    n, K = 2, 64
    case = helpers.build_case("drn_d_22_unary", 128, 256, 32, seed=3, n_images=n)
    cfg = case["cfg"]
    Hs, Ws, P2S = cfg.rows // 8, cfg.realcols, case["segmentation"].shape[-1]
    assert (Hs, Ws, cfg.cols) == (16, 32, 256)
    f, w, b = hr.random_inputs(n, K, Hs, Ws, 21, seed=5)
    st = host.Stixels()
    st.SetConfig(cfg)
    st.Initialize(max_batch=n)
    st.SetSegmentationHead(w, b, K)
    d_f = torch.from_numpy(f).to(dev)
    d_seg = torch.empty((n, Ws, 21, P2S), dtype=torch.int32, device=dev)
    d_cnn = torch.empty((n, 21, Hs, Ws), dtype=torch.float32, device=dev)
    d_gt = torch.from_numpy(_gt(n, 8 * Hs, 8 * Ws, seed=6)).to(dev)
    d_label = torch.full((n, 8 * Hs, 8 * Ws), 0xA5, dtype=torch.uint8, device=dev)
    d_c8 = torch.full((n, Hs, Ws), 0xA5, dtype=torch.uint8, device=dev)
    d_conf = torch.zeros((NL, NL), dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    st.SegmentationHeadBatch(n, d_f.data_ptr(), core.HEAD_F32, d_seg.data_ptr(), d_cnn.data_ptr(), stream)
    st.CnnLabelBatch(n, d_cnn.data_ptr(), core.CNN_UP_MODES[mode], d_class8=d_c8.data_ptr(), d_label=d_label.data_ptr(),
                     d_gt_label=d_gt.data_ptr(), n_labels=NL, d_confusion=d_conf.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert st.LastFrames() == 0                                              # a producer, not a compute call
    direct = core.cnn_label_maps(d_cnn, 19, mode=mode, gt_label=d_gt, want_class8=True)
    assert torch.equal(direct["label"], d_label) and torch.equal(direct["class8"], d_c8)
    assert torch.equal(direct["confusion"], d_conf) and int(d_conf.sum()) > 0
    with pytest.raises(ValueError, match="n_images"):
        st.CnnLabelBatch(n + 1, d_cnn.data_ptr(), core.CNN_UP_NEAREST, d_label=d_label.data_ptr())
    with pytest.raises(ValueError, match="mode"):
        st.CnnLabelBatch(n, d_cnn.data_ptr(), 7, d_label=d_label.data_ptr())
    with pytest.raises(ValueError, match="go together"):
        st.CnnLabelBatch(n, d_cnn.data_ptr(), core.CNN_UP_NEAREST, d_label=d_label.data_ptr(),
                         d_gt_label=d_gt.data_ptr())
    st.close()


@pytest.mark.parametrize("mode", MODES)
def test_cnn_scores_accumulate_over_half_batches(mode):
    torch, dev = _torch()
    x = cr.random_costs(4, 21, 5, 7, seed=31)
    gt = cr.label_maps(x, 19, "nearest")[1].copy()                           # a ground truth the CNN partly meets
    rng = np.random.default_rng(32)
    noise = rng.random(gt.shape) < 0.3
    gt[noise] = cr.CITYSCAPES[rng.integers(0, 19, int(noise.sum()))]
    d_x, d_gt = torch.from_numpy(x).to(dev), torch.from_numpy(gt).to(dev)
    whole = evaluation.cnn_scores(d_x, d_gt, mode=mode)
    first = evaluation.cnn_scores(d_x[:2], d_gt[:2], mode=mode)
    both = evaluation.cnn_scores(d_x[2:], d_gt[2:], mode=mode, confusion=first["confusion"])
    assert torch.equal(both["confusion"], whole["confusion"])
    assert np.array_equal(both["iou"], whole["iou"], equal_nan=True) and both["mean_iou"] == whole["mean_iou"]
    want = cr.confusion(cr.label_maps(x, 19, mode)[1], gt, NL, 56)
    assert np.array_equal(whole["confusion"].cpu().numpy().astype(np.uint64), want)
    iou, mean = evaluation.cityscapes_iou(want)
    assert whole["mean_iou"] == mean and 0.0 < mean < 1.0
