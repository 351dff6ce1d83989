"""f5 on the MI355X: Stixels::RenderBatch / is_render_sections (is_k_render.hip) against the numpy restatement
of tests/render_reference.py, fed from the Sections and instance mappings the same compute call returned.
Images are compared exactly (the disparity bit for bit), the confusion matrix exactly, the deviation sums to
1e-9 relative with exact counts; canary bytes around every output must survive."""
import ctypes

import numpy as np
import pytest

import helpers
import render_reference as rr
from instance_stixels_amd import core, host, synthetic
from instance_stixels_amd.config import SECTION_DTYPE

pytestmark = pytest.mark.gpu

PAD = 256          # canary bytes in front of and behind every output
CANARY = 0xA5
N_LABELS = 34

# (rows, cols, max_dis, n, overrides): the shapes of the issue; 64x72 with width_margin 8 has w = 72 // 8 = 9
SHAPES = [(256, 512, 64, 4, {}), (1024, 2048, 128, 8, {}), (784, 1792, 128, 2, dict(invalid_disparity=0.0)),
          (64, 72, 32, 2, dict(width_margin=8))]
PRESETS = ["drn_d_22_unary", "drn_d_38_pairwise"]


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


class Out:
    """A device buffer of `shape` x `dtype` with canaries around it; the body starts as garbage."""

    def __init__(self, shape, dtype, fill=0x5C, offset=0):
        torch, dev = _torch()
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.off = PAD + offset
        self.buf = torch.full((self.nbytes + 2 * PAD + offset,), CANARY, dtype=torch.uint8, device=dev)
        self.buf[self.off:self.off + self.nbytes] = fill
        self.ptr = self.buf.data_ptr() + self.off

    def get(self):
        b = self.buf.cpu().numpy()
        assert (b[:self.off] == CANARY).all() and (b[self.off + self.nbytes:] == CANARY).all(), "canary overwritten"
        return b[self.off:self.off + self.nbytes].view(self.dtype).reshape(self.shape).copy()


def _dev(a):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _ground_truth(label, disp, seed):
    """gt labels: the rendered labels with noise, 255s and ids >= N_LABELS mixed in; gt disparity: the rendered
    disparity with noise, zeros, and values where the stixels have none."""
    rng = np.random.default_rng(seed)
    gt = label.copy()
    r = rng.random(gt.shape)
    gt[r < 0.10] = rng.integers(0, 40, int((r < 0.10).sum()))
    gt[(r >= 0.10) & (r < 0.15)] = 255
    gd = (disp + rng.normal(0, 0.7, disp.shape)).astype(np.float32)
    gd[rng.random(gd.shape) < 0.2] = 0.0
    empty = disp == 0
    gd[empty] = rng.uniform(0, 50, int(empty.sum())).astype(np.float32)
    return gt, gd


def _full(st, n, shape, gt, gd, stream=0):
    """RenderBatch with every output; returns (label, disparity, instance, confusion, sums, counts, stixels)."""
    lab, dsp, ins = Out(shape, np.uint8), Out(shape, np.float32), Out(shape, np.int32)
    conf = Out((N_LABELS, N_LABELS), np.uint64, fill=0)
    d_gt, d_gd = _dev(gt), _dev(gd)
    _torch()[0].cuda.synchronize()
    s, c, k = st.RenderBatch(n, label=lab.ptr, disparity=dsp.ptr, instance=ins.ptr, gt_label=d_gt.data_ptr(),
                             n_labels=N_LABELS, confusion=conf.ptr, gt_disparity=d_gd.data_ptr(), stream=stream)
    return lab.get(), dsp.get(), ins.get(), conf.get(), s, c, k


def _check(got, want_imgs, gt, gd, rows, cols, realcols):
    label, disp, inst, conf, s, c, k = got
    wl, wd, wi, wk = want_imgs
    np.testing.assert_array_equal(label, wl)
    np.testing.assert_array_equal(disp.view(np.int32), wd.view(np.int32))
    np.testing.assert_array_equal(inst, wi)
    w = cols // realcols
    assert (label[:, :, :realcols * w] != 0).all(), "a stixel pixel was left uncovered"
    assert not label[:, :, realcols * w:].any() and not disp[:, :, realcols * w:].any()
    np.testing.assert_array_equal(conf, rr.confusion(wl, gt, N_LABELS))
    ws, wc = rr.deviation(wd, gd)
    np.testing.assert_array_equal(c, wc)
    np.testing.assert_allclose(s, ws, rtol=1e-9, atol=0)
    np.testing.assert_array_equal(k, wk)


def _setup(preset, rows, cols, D, n, ov, seed):
    torch, dev = _torch()
    ov = dict(ov, size_filter=10 if preset.endswith("unary") else 8)
    case = helpers.build_case(preset, rows, cols, D, seed=seed, n_images=n, **ov)
    cfg = case["cfg"]
    # frames with instance offsets, so that clusters form (as test_f1_f2's batched instance test)
    frames = [synthetic.make_frame(cfg, seed=seed + 100 * i, n_slabs=10 + 2 * i, offset_scale=1.0)
              for i in range(n)]
    case["frames"] = frames
    case["disparity"] = np.stack([f.disparity for f in frames])
    case["segmentation"] = np.stack([f.segmentation for f in frames])
    st = host.Stixels()
    st.SetConfig(cfg)
    st.Initialize(max_batch=n)
    big, seg = _dev(case["disparity"]), _dev(case["segmentation"])
    road = [(f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground) for f in case["frames"]]
    data, maps = st.ComputeBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), road, with_instances=True)
    secs = np.stack([d.sections for d in data])
    return st, case, (big, seg, road), secs, maps


@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("rows, cols, D, n, ov", SHAPES)
def test_render_batch_matches_restatement(preset, rows, cols, D, n, ov):
    st, case, _, secs, maps = _setup(preset, rows, cols, D, n, ov, seed=rows + n)
    realcols = st.GetRealCols()
    want = rr.render(secs, rows, cols, maps)
    gt, gd = _ground_truth(want[0], want[1], seed=cols)
    got = _full(st, n, (n, rows, cols), gt, gd)
    _check(got, want, gt, gd, rows, cols, realcols)
    if rows >= 256:
        assert (want[2] != 0).any(), "no instance pixels: the case does not exercise the instance image"
    # a smaller render of the same call: the first frame only
    got1 = _full(st, 1, (1, rows, cols), gt[:1], gd[:1])
    _check(got1, tuple(x[:1] for x in want), gt[:1], gd[:1], rows, cols, realcols)
    st.close()


@pytest.mark.parametrize("preset", PRESETS)
def test_render_after_compute_single_frame(preset):
    rows, cols, D = 256, 512, 64
    case = helpers.build_case(preset, rows, cols, D, seed=5, size_filter=10 if preset.endswith("unary") else 8)
    cfg = case["cfg"]
    f = synthetic.make_frame(cfg, seed=5, n_slabs=16, offset_scale=1.0)
    st = host.Stixels()
    st.SetConfig(cfg)
    st.Initialize()
    st.SetDisparityImage(f.disparity)
    st.SetSegmentation(f.segmentation)
    st.SetRoadParameters(f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground)
    data = st.Compute(cfg.pairwise)
    mapping = st.GetInstanceStixels()
    want = rr.render(data.sections[None], rows, cols, [mapping])
    gt, gd = _ground_truth(want[0], want[1], seed=9)
    _check(_full(st, 1, (1, rows, cols), gt, gd), want, gt, gd, rows, cols, st.GetRealCols())
    assert (want[2] != 0).any()
    with pytest.raises(ValueError, match="n_images"):
        st.RenderBatch(2)
    st.close()


def test_render_is_deterministic_subsets_agree_streams_and_refusals():
    torch, dev = _torch()
    rows, cols, D, n = 256, 512, 64, 4
    st, case, (big, seg, road), secs, maps = _setup("drn_d_38_pairwise", rows, cols, D, n, {}, seed=3)
    want = rr.render(secs, rows, cols, maps)
    gt, gd = _ground_truth(want[0], want[1], seed=4)
    d_gt, d_gd = _dev(gt), _dev(gd)
    shape = (n, rows, cols)
    full = _full(st, n, shape, gt, gd)
    # two calls into one confusion buffer: the same bits for the sums, exactly twice the counts
    conf = Out((N_LABELS, N_LABELS), np.uint64, fill=0)
    r1 = st.RenderBatch(n, gt_label=d_gt.data_ptr(), confusion=conf.ptr, gt_disparity=d_gd.data_ptr())
    r2 = st.RenderBatch(n, gt_label=d_gt.data_ptr(), confusion=conf.ptr, gt_disparity=d_gd.data_ptr())
    assert r1[0].tobytes() == r2[0].tobytes() == full[4].tobytes()
    np.testing.assert_array_equal(r1[1], full[5])
    np.testing.assert_array_equal(conf.get(), 2 * full[3])
    # every output alone gives what the full call gave
    for name, dtype, idx in (("label", np.uint8, 0), ("disparity", np.float32, 1), ("instance", np.int32, 2)):
        o = Out(shape, dtype)
        s, c, k = st.RenderBatch(n, **{name: o.ptr})
        assert o.get().tobytes() == full[idx].tobytes(), name
        assert not s.any() and not c.any()
        np.testing.assert_array_equal(k, full[6])
    conf = Out((N_LABELS, N_LABELS), np.uint64, fill=0)
    st.RenderBatch(n, gt_label=d_gt.data_ptr(), confusion=conf.ptr)
    np.testing.assert_array_equal(conf.get(), full[3])
    s, c, k = st.RenderBatch(n, gt_disparity=d_gd.data_ptr())
    assert s.tobytes() == full[4].tobytes()
    np.testing.assert_array_equal(c, full[5])
    # a misaligned label image (the per-pixel path) and a custom class table with a smaller n_labels
    o = Out(shape, np.uint8, offset=3)
    table = np.arange(19, dtype=np.uint8) + 1
    conf = Out((20, 20), np.uint64, fill=0)
    st.RenderBatch(n, label=o.ptr, gt_label=d_gt.data_ptr(), n_labels=20, confusion=conf.ptr,
                   class_to_label=table)
    want_t = rr.render(secs, rows, cols, maps, class_to_label=table)[0]
    np.testing.assert_array_equal(o.get(), want_t)
    np.testing.assert_array_equal(conf.get(), rr.confusion(want_t, gt, 20))
    # a non-default stream
    stream = torch.cuda.Stream(device=dev)
    got = _full(st, n, shape, gt, gd, stream=stream.cuda_stream)
    for a, b in zip(got, full):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    # refusals: too many frames, an instance image of a call without instances, a bad n_labels
    with pytest.raises(ValueError, match="n_images"):
        st.RenderBatch(n + 1)
    with pytest.raises(ValueError, match="n_labels"):
        st.RenderBatch(n, gt_label=d_gt.data_ptr(), n_labels=65, confusion=conf.ptr)
    st.ComputeBatch(True, big.data_ptr(), seg.data_ptr(), road[:2], with_instances=False)
    with pytest.raises(ValueError, match="instance"):
        st.RenderBatch(2, instance=Out(shape, np.int32).ptr)
    lab = Out((2, rows, cols), np.uint8)
    st.RenderBatch(2, label=lab.ptr)
    np.testing.assert_array_equal(lab.get(), want[0][:2])    # (the same frames, the same Sections)
    st.close()


def _hostile_sections(rows, realcols, S, rng):
    """Three frames: frame 0 well-formed (a partition of every column), frame 1 hostile columns next to
    well-formed ones, frame 2 empty columns only."""
    secs = np.zeros((3, realcols, S), SECTION_DTYPE)
    secs["type"] = -1

    def partition(col, cuts, classes):
        v = 0
        for k, (cut, cls) in enumerate(zip(cuts, classes)):
            col[k] = (k % 3, v, cut - 1, rng.uniform(0.5, 60), cls, 0, 0, 0)
            v = cut
        col[len(cuts)] = (-1, 0, 0, 0, 0, 0, 0, 0)

    for f in range(2):
        for c in range(realcols):
            k = int(rng.integers(1, 12))
            cuts = sorted(rng.choice(np.arange(1, rows), k - 1, replace=False).tolist()) + [rows]
            partition(secs[f, c], cuts, rng.integers(0, 19, k))
    hostile = {}
    c = 0
    secs[1, c, 0]["type"] = -1                           # an empty column
    hostile[c] = "empty"; c += 1
    partition(secs[1, c], list(range(1, 200)), rng.integers(0, 19, 199))   # 199 one-row sections
    hostile[c] = "199 one-row"; c += 1
    ent = [(1, 5, 40, 3.0, 11), (1, 20, 60, 4.0, 12), (0, -30, 10, 5.0, 0), (2, rows - 5, rows + 100, 6.0, 10),
           (1, 50, 10, 7.0, 13), (1, -2**31, 2**31 - 1, 8.0, 14), (1, 2**31 - 1, -2**31, 9.0, 15),
           (1, rows + 5, rows + 9, 1.0, 1), (1, -9, -5, 1.0, 2)]
    for k, (t, vb, vt, d, cls) in enumerate(ent):           # overlapping and out-of-range entries
        secs[1, c, k] = (t, vb, vt, d, cls, 0, 0, 0)
    secs[1, c, len(ent)]["type"] = -1
    hostile[c] = "overlap / out of range"; c += 1
    partition(secs[1, c], [10, 30, rows], [-5, 19, 100000])  # classes outside the table
    hostile[c] = "classes outside the table"; c += 1
    for k in range(S):                                      # no terminator at all
        secs[1, c, k] = (1, k, k, 2.0, 3, 0, 0, 0)
    hostile[c] = "no terminator"
    return secs, hostile


@pytest.mark.parametrize("rows, realcols, cols", [(256, 64, 512), (250, 70, 565), (199, 5, 67)])
def test_hostile_sections_through_the_c_abi(rows, realcols, cols):
    """Hand-built Sections straight into is_render_sections (no instances): no fault, no write outside the
    outputs, and the well-formed columns of the same batch exact.  The 8-pixel vector path (w = 8, cols % 8 == 0)
    and the per-pixel path (cols % 8 != 0; w = 8 and 13) both."""
    torch, dev = _torch()
    S = 200
    rng = np.random.default_rng(rows + realcols)
    secs, hostile = _hostile_sections(rows, realcols, S, rng)
    n = secs.shape[0]
    d_secs = _dev(secs.view(np.uint8))
    want = rr.render(secs, rows, cols, None)
    gt, gd = _ground_truth(want[0], want[1], seed=1)
    d_gt, d_gd = _dev(gt), _dev(gd)
    shape = (n, rows, cols)
    lab, dsp, ins = Out(shape, np.uint8), Out(shape, np.float32), Out(shape, np.int32)
    conf = Out((N_LABELS, N_LABELS), np.uint64, fill=0)
    sums, cnts, nst = Out((n,), np.float64), Out((n,), np.int64), Out((n,), np.int32)
    torch.cuda.synchronize()
    core.render_sections_ptr(d_sections=d_secs.data_ptr(), n_images=n, realcols=realcols, max_sections=S,
                             rows=rows, cols=cols, d_label=lab.ptr, d_disparity=dsp.ptr, d_instance=ins.ptr,
                             d_gt_label=d_gt.data_ptr(), n_labels=N_LABELS, d_confusion=conf.ptr,
                             d_gt_disparity=d_gd.data_ptr(), d_disp_abs_sum=sums.ptr, d_disp_count=cnts.ptr,
                             d_stixel_count=nst.ptr)
    torch.cuda.synchronize()
    label, disp, inst = lab.get(), dsp.get(), ins.get()
    assert not inst.any()
    w = cols // realcols
    well = [c for c in range(realcols) if c not in hostile]
    for c in well:       # frames 0 and 1: the well-formed columns exactly
        xs = slice(c * w, c * w + w)
        np.testing.assert_array_equal(label[:, :, xs], want[0][:, :, xs])
        np.testing.assert_array_equal(disp[:, :, xs].view(np.int32), want[1][:, :, xs].view(np.int32))
    np.testing.assert_array_equal(label[0], want[0][0])
    np.testing.assert_array_equal(label[2], want[0][2])
    assert not label[:, :, realcols * w:].any()
    # hostile columns: the kernel paints in section order like the restatement, so they agree too
    np.testing.assert_array_equal(label, want[0])
    np.testing.assert_array_equal(disp.view(np.int32), want[1].view(np.int32))
    np.testing.assert_array_equal(conf.get(), rr.confusion(want[0], gt, N_LABELS))
    ws, wc = rr.deviation(want[1], gd)
    np.testing.assert_array_equal(cnts.get(), wc)
    np.testing.assert_allclose(sums.get(), ws, rtol=1e-9, atol=0)
    np.testing.assert_array_equal(nst.get(), want[3])
    # the per-section instance map of hand-made candidate arrays: out-of-range (column, section) pairs skipped
    L = core.lib()
    CS = realcols * S
    idx = np.full((8, CS, 2), -1, np.int32)
    lbl = np.full((8, CS), -1, np.int32)
    per = np.zeros(8, np.int32)
    cand = [(0, 0, 4), (0, 1, 1000), (realcols - 1, 2, 7), (realcols, 0, 5), (0, S, 5), (-1, 3, 5)]
    for j, (u, v, l) in enumerate(cand):
        idx[3, j], lbl[3, j] = (u, v), l
    per[3] = len(cand)
    per[5] = -7                  # a negative count is none
    d_idx, d_lbl, d_per = _dev(idx), _dev(lbl), _dev(per)
    ib = (core.InstanceBuffers * 1)()
    ib[0].d_indices, ib[0].d_labels, ib[0].d_instances_per_class = d_idx.data_ptr(), d_lbl.data_ptr(), d_per.data_ptr()
    m = Out((1, realcols, S), np.int32)
    assert L.is_section_instance_labels(ib, 1, realcols, S, ctypes.c_void_p(m.ptr), None) == 0
    torch.cuda.synchronize()
    got = m.get()
    want_m = np.full((1, realcols, S), -1, np.int32)
    want_m[0, 0, 0], want_m[0, 0, 1], want_m[0, realcols - 1, 2] = 4, 1000, 7
    np.testing.assert_array_equal(got, want_m)
