"""f11 on the MI355X: is_mode_downsample, is_gt_instance_targets (is_k_gt_targets.hip), core.gt_instance_targets and
Stixels::GroundTruthOffsetsBatch against the numpy restatement of tests/gt_targets_reference.py and the reference's own
Python (tests/golden/reference_python_targets), bit for bit.  Canary bytes around every buffer of the C ABI, the
scratch included, must survive."""
import numpy as np
import pytest

import gt_targets_reference as gr
import helpers
from instance_stixels_amd import core, evaluation, host, synthetic
from test_gt_targets import GOLDEN, bits, fixture_case
from test_render_gpu import Out, _dev, _torch

pytestmark = pytest.mark.gpu
FILL = 0x5C   # the garbage Out() starts with


def _scene(n, rows, cols, seed, ids=None):
    """Cityscapes-like instanceIds [n][rows][cols] int32 and raw disparities uint16: blobs whose borders do not follow
    the 8x8 blocks, on stuff labels; disparities with holes."""
    rng = np.random.default_rng(seed)
    stuff = np.array([7, 8, 11, 21, 23, 1000], np.int32)
    gt = stuff[rng.integers(0, stuff.size, (n, rows // 16 + 1, cols // 16 + 1))].repeat(16, 1).repeat(16, 2)
    gt = np.ascontiguousarray(gt[:, :rows, :cols])
    disp = (rng.integers(0, 3, gt.shape) * 5000).astype(np.uint16)
    pool = np.array(ids if ids is not None else [24001, 24002, 26001, 26002, 26003, 33001, 29001, 13004, 1001], np.int32)
    for f in range(n):
        for k in range(int(rng.integers(6, 14))):
            h, w = int(rng.integers(1, max(2, rows // 2))), int(rng.integers(1, max(2, cols // 3)))
            y0, x0 = int(rng.integers(0, rows - h + 1)), int(rng.integers(0, cols - w + 1))
            yy, xx = np.mgrid[0:h, 0:w]
            blob = ((yy - h / 2) / (h / 2)) ** 2 + ((xx - w / 2) / (w / 2)) ** 2 <= 1.0
            gt[f, y0:y0 + h, x0:x0 + w][blob] = pool[int(rng.integers(0, pool.size))]
            q = int(rng.integers(0, 200))
            disp[f, y0:y0 + h, x0:x0 + w][blob] = (q * 256 + (yy[blob] % 4) * 256 * (k % 2) + 77) % 65536
    return gt, disp


def _p2s(rows):
    p = 1
    while p < rows // 8 + 1:
        p *= 2
    return p


def _shifted(a, offset):
    """A device copy of `a` that starts `offset` bytes into a larger buffer."""
    torch, dev = _torch()
    b = np.ascontiguousarray(a).view(np.uint8).ravel()
    raw = torch.zeros(b.size + 64, dtype=torch.uint8, device=dev)
    raw[offset:offset + b.size] = _dev(b)
    return raw, raw.data_ptr() + offset


def _c_abi(gt, disp=None, planes=2, seg=None, capacity=0, gt_offset=0, want_ids=True, want_targets=True):
    """is_gt_instance_targets on host arrays with canaries around every output and the scratch.  seg: the tensor the
    call rewrites ([n][Ws][21][P2S] int32).  Returns dict(rc, targets, ids8, seg, count) as numpy."""
    torch, dev = _torch()
    n, rows, cols = gt.shape
    Hs, Ws = rows // 8, cols // 8
    keep_gt, p_gt = _shifted(np.asarray(gt, np.int32), gt_offset)
    keep_d, p_d = _shifted(np.asarray(disp, np.uint16), 0) if disp is not None else (None, None)
    t = Out((n, planes, Hs, Ws), np.float32) if want_targets else None
    i8 = Out((n, Hs, Ws), np.int32) if want_ids else None
    cnt = Out((n,), np.int32)
    s = None
    if seg is not None:
        s = Out(seg.shape, np.int32)
        s.buf[s.off:s.off + s.nbytes] = _dev(np.ascontiguousarray(seg, np.int32).view(np.uint8).ravel())
    nbytes = core.gt_targets_scratch_bytes(n, rows, cols, disp is not None, capacity)
    assert nbytes > 0
    scratch = Out((nbytes,), np.uint8, offset=0)
    assert scratch.ptr % 16 == 0
    torch.cuda.synchronize()
    rc = core.gt_instance_targets_ptr(
        d_gt_instance=p_gt, d_disparity_u16=p_d, n_images=n, rows=rows, cols=cols,
        d_targets=t.ptr if t else None, target_planes=planes if t else 0, d_ids8=i8.ptr if i8 else None,
        d_segmentation=s.ptr if s else None, rows_power2_segmentation=seg.shape[3] if s else 0,
        channels=21 if s else 0, capacity=capacity, d_scratch=scratch.ptr, scratch_bytes=nbytes, d_key_count=cnt.ptr)
    torch.cuda.synchronize()
    scratch.get()
    assert (keep_gt[:gt_offset] == 0).all().item() and (keep_gt[gt_offset + gt.size * 4:] == 0).all().item()
    return dict(rc=rc, targets=t.get() if t else None, ids8=i8.get() if i8 else None, seg=s.get() if s else None,
                count=cnt.get())


def _want(gt, disp=None, seg=None):
    t, i8 = gr.targets(gt, disp)
    return dict(targets=t, ids8=i8, count=gr.key_counts(i8),
                seg=gr.as_prediction(seg, t[:, -2:]) if seg is not None else None)


def _same(got, want, what=""):
    assert got["rc"] == 0, core.lib().is_last_error()
    for k in ("ids8", "count", "seg"):
        if got[k] is not None:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what} {k}")
    if got["targets"] is not None:
        np.testing.assert_array_equal(bits(got["targets"]), bits(want["targets"]), err_msg=f"{what} targets")


def _garbage_seg(n, rows, cols, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-2**31, 2**31 - 1, (n, cols // 8, 21, _p2s(rows)), dtype=np.int64).astype(np.int32)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_c_abi_on_the_fixture_cases(k):
    """The cases of the reference's own Python, one frame and three: targets with 2 and 3 planes, ids, segmentation."""
    gt, disp, ids8, d8, t3 = fixture_case(np.load(GOLDEN), k)
    rows, cols = gt.shape
    seg = _garbage_seg(1, rows, cols, k)
    got = _c_abi(gt[None], disp[None], planes=3, seg=seg)
    _same(got, _want(gt[None], disp[None], seg), "3 planes")
    np.testing.assert_array_equal(bits(got["targets"][0]), bits(t3))          # the reference itself
    np.testing.assert_array_equal(got["ids8"][0], ids8)
    got = _c_abi(gt[None], planes=2, seg=seg)
    _same(got, _want(gt[None], None, seg), "2 planes")
    np.testing.assert_array_equal(bits(got["targets"][0]), bits(t3[1:]))
    _same(_c_abi(gt[None], disp[None], planes=2), _want(gt[None]), "2 planes with a disparity image")
    # three frames: the fixture, upside down, and shifted by three cells and a bit
    gt3 = np.stack([gt, gt[::-1], np.roll(gt, (27, 13), (0, 1))])
    d3 = np.stack([disp, disp[::-1], np.roll(disp, (27, 13), (0, 1))])
    seg3 = _garbage_seg(3, rows, cols, k + 10)
    _same(_c_abi(gt3, d3, planes=3, seg=seg3), _want(gt3, d3, seg3), "three frames")
    _same(_c_abi(gt3, planes=2, seg=seg3, want_ids=False), _want(gt3, None, seg3), "three frames, no ids")
    _same(_c_abi(gt3, seg=seg3, want_ids=False, want_targets=False), _want(gt3, None, seg3), "segmentation alone")


@pytest.mark.parametrize("rows, cols", [(64, 128), (72, 520), (8, 8), (528, 72), (136, 1032)])
def test_c_abi_shapes_at_the_kernels_edges(rows, cols):
    """8x16 cells (less than a wave), Ws = 65 (one tail lane, two tiles across), one cell, Hs = 66 (two tiles down),
    Ws = 129 (three chunks); a misaligned ground truth (the per-pixel path) gives the aligned result."""
    gt, disp = _scene(2, rows, cols, seed=rows + cols)
    seg = _garbage_seg(2, rows, cols, rows)
    want = _want(gt, disp, seg)
    if rows > 8:
        assert want["count"].min() >= 2 and (want["ids8"] > 1000).any() and (want["ids8"] <= 1000).any()
    aligned = _c_abi(gt, disp, planes=3, seg=seg)
    _same(aligned, want, "aligned")
    _same(_c_abi(gt, disp, planes=3, seg=seg, gt_offset=4), want, "offset by 4 bytes")
    if rows == 8:   # the one cell as an instance
        gt[...] = 26001
        got = _c_abi(gt, planes=2, seg=seg)
        _same(got, _want(gt, None, seg))
        assert (got["targets"] == 0).all() and got["count"].tolist() == [1, 1]


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int32])
def test_mode_downsample_types_alignment_and_ties(dtype):
    """core.mode_downsample on the three types: random blocks of few values (ties are frequent), uniform blocks, values
    at the ends of the type's range; the aligned and the per-element path."""
    torch, dev = _torch()
    rng = np.random.default_rng(np.dtype(dtype).itemsize)
    info = np.iinfo(dtype)
    pool = np.array([info.min, info.min + 1, info.max, info.max - 1, 7, 100], dtype)
    img = pool[rng.integers(0, pool.size, (3, 40, 520))]
    img[:, :16] = img[:, :1, :1]                                   # uniform blocks: the fast path
    img[1, 16:24, :] = np.arange(520, dtype=np.int64).astype(dtype)[None, :]   # eight values of eight pixels each
    want = gr.mode_downsample(img)
    t = _dev(img)
    got = core.mode_downsample(t)
    assert got.dtype == t.dtype and got.device == t.device
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    np.testing.assert_array_equal(core.mode_downsample(t[0]).cpu().numpy(), want[0])
    keep, ptr = _shifted(img, img.itemsize)                        # off the 16-byte alignment by one element
    out = Out(want.shape, dtype)
    torch.cuda.synchronize()
    code = {np.uint8: core.DTYPE_UINT8, np.uint16: core.DTYPE_UINT16, np.int32: core.DTYPE_INT32}[dtype]
    assert core.mode_downsample_ptr(ptr, code, 3, 40, 520, out.ptr) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.get(), want)


def test_segmentation_write_against_flip_and_pad():
    """The class channels are bit-identical before and after, the padding rows of channels 19 and 20 are zero whatever
    the buffer held, and the tensor equals is_flip_and_pad of the CNN output whose last two channels are the
    restatement's offsets."""
    n, rows, cols = 2, 136, 264
    Hs, Ws, P2S = rows // 8, cols // 8, _p2s(rows)
    gt, _ = _scene(n, rows, cols, seed=11)
    rng = np.random.default_rng(3)
    cnn = rng.normal(0, 3, (n, 21, Hs, Ws)).astype(np.float32)
    seg = core.flip_and_pad(cnn, P2S)
    seg[:, :, 19:, :] = rng.integers(-2**31, 2**31 - 1, seg[:, :, 19:, :].shape, dtype=np.int64).astype(np.int32)
    got = _c_abi(gt, seg=seg, want_targets=False)
    assert got["rc"] == 0
    np.testing.assert_array_equal(got["seg"][:, :, :19], seg[:, :, :19])
    assert (got["seg"][:, :, 19:, Hs:] == 0).all()
    off, _ = gr.targets(gt)
    assert (off != 0).any() and (np.float32(8) * off < 0).any()
    replaced = cnn.copy()
    replaced[:, 19:] = off
    np.testing.assert_array_equal(got["seg"], core.flip_and_pad(replaced, P2S))
    # the torch entry point, in place on the caller's tensor
    t = _dev(seg)
    targets, ids8 = core.gt_instance_targets(_dev(gt), segmentation=t)
    np.testing.assert_array_equal(t.cpu().numpy(), got["seg"])
    np.testing.assert_array_equal(bits(targets.cpu().numpy()), bits(off))


def test_hostile_ids_stay_inside_their_buffers_and_repeat():
    """Negative ids, INT32_MAX, a new id per cell (keys = cells): the restatement's bytes, canaries intact (checked by
    _c_abi), the same bytes on two runs."""
    n, rows, cols = 2, 72, 520
    Hs, Ws = rows // 8, cols // 8
    rng = np.random.default_rng(9)
    per_cell = (2000 + np.arange(Hs * Ws, dtype=np.int32).reshape(Hs, Ws) * 7919 % 2**20).repeat(8, 0).repeat(8, 1)
    assert np.unique(per_cell).size == Hs * Ws
    wild = rng.choice(np.array([-1, -2**31, 2**31 - 1, 2**31 - 2, -26001, 1000, 1001, 0], np.int32), (rows, cols))
    gt = np.stack([per_cell, wild]).astype(np.int32)
    disp = rng.integers(0, 65536, gt.shape).astype(np.uint16)
    seg = _garbage_seg(n, rows, cols, 1)
    want = _want(gt, disp, seg)
    assert want["count"].tolist()[0] == Hs * Ws and (want["ids8"][1] == 2**31 - 1).any() and (want["ids8"][1] < 0).any()
    first = _c_abi(gt, disp, planes=3, seg=seg, capacity=Hs * Ws)
    _same(first, want)
    again = _c_abi(gt, disp, planes=3, seg=seg, capacity=Hs * Ws)
    for k in ("targets", "ids8", "seg", "count"):
        assert first[k].tobytes() == again[k].tobytes(), k
    _same(_c_abi(gt, planes=2, seg=seg), _want(gt, None, seg), "without the disparity the capacity does not matter")


def test_more_keys_than_the_capacity_writes_nothing_and_reports_the_count():
    """Frame 1 has 40 keys, the others 3 and 5: with a capacity of 16 no output of any frame is touched and the true
    counts are reported; the torch entry point repeats with that count and returns the complete result."""
    n, rows, cols = 3, 64, 128
    gt = np.full((n, rows, cols), 7, np.int32)
    for f, keys in enumerate((3, 40, 5)):
        for k in range(keys):
            gt[f, 8 * (k // 8):8 * (k // 8) + 8, 16 * (k % 8):16 * (k % 8) + 16] = 26001 + k
    disp = np.full(gt.shape, 30 * 256, np.uint16)
    disp[1, :, 64:] = 90 * 256
    seg = _garbage_seg(n, rows, cols, 2)
    want = _want(gt, disp, seg)
    assert want["count"].tolist() == [3, 40, 5]
    got = _c_abi(gt, disp, planes=3, seg=seg, capacity=16)
    assert got["rc"] == 0 and got["count"].tolist() == [3, 40, 5]
    assert (got["targets"].view(np.uint8) == FILL).all() and (got["ids8"].view(np.uint8) == FILL).all()
    np.testing.assert_array_equal(got["seg"], seg)
    _same(_c_abi(gt, disp, planes=3, seg=seg, capacity=40), want, "exactly enough")
    _same(_c_abi(gt[[0, 2]], disp[[0, 2]], planes=3, seg=seg[[0, 2]], capacity=16),
          _want(gt[[0, 2]], disp[[0, 2]], seg[[0, 2]]), "the other frames alone fit")
    torch, dev = _torch()
    t_seg = _dev(seg)
    targets, ids8, count = core.gt_instance_targets(_dev(gt), _dev(disp), segmentation=t_seg, capacity=16,
                                                    return_key_count=True)
    np.testing.assert_array_equal(bits(targets.cpu().numpy()), bits(want["targets"]))
    np.testing.assert_array_equal(ids8.cpu().numpy(), want["ids8"])
    np.testing.assert_array_equal(t_seg.cpu().numpy(), want["seg"])
    assert count.cpu().numpy().tolist() == [3, 40, 5]


def test_host_class_offsets_then_compute_batch_equals_the_oracle():
    """GroundTruthOffsetsBatch is legal before any compute call and leaves the consumers' refusals in place; then
    ComputeBatch on the rewritten tensor gives the Sections the oracle gives on the restatement's tensor."""
    torch, dev = _torch()
    n, rows, cols, D = 2, 256, 1024, 64
    case = helpers.build_case("drn_d_22_unary", rows, cols, D, seed=5, n_images=n, size_filter=12, eps=23.89408, min_pts=4)
    cfg = case["cfg"]
    frames = [synthetic.make_frame(cfg, seed=5 + 100 * i, n_slabs=12, offset_scale=1.0) for i in range(n)]
    case["frames"] = frames
    case["disparity"] = np.stack([f.disparity for f in frames])
    case["segmentation"] = np.stack([f.segmentation for f in frames])
    gt, _ = _scene(n, rows, cols, seed=21)
    off, _ = gr.targets(gt)
    want_seg = gr.as_prediction(case["segmentation"], off)
    assert (want_seg != case["segmentation"]).any()
    st = host.Stixels()
    st.SetConfig(cfg)
    st.Initialize(max_batch=n)
    big, seg, d_gt = _dev(case["disparity"]), _dev(case["segmentation"]), _dev(gt)
    st.GroundTruthOffsetsBatch(n, d_gt.data_ptr(), seg.data_ptr())               # before any compute call
    torch.cuda.synchronize()
    np.testing.assert_array_equal(seg.cpu().numpy(), want_seg)
    with pytest.raises(ValueError, match="there are none"):
        st.InstanceOverlapBatch(n, d_gt.data_ptr())
    with pytest.raises(ValueError, match="there are none"):
        st.AssignInstancesGTBatch(n, d_gt.data_ptr())
    assert st.LastFrames() == 0
    with pytest.raises(ValueError, match="n_images"):
        st.GroundTruthOffsetsBatch(n + 1, d_gt.data_ptr(), seg.data_ptr())
    with pytest.raises(ValueError, match="null"):
        st.GroundTruthOffsetsBatch(n, 0, seg.data_ptr())
    road = [(f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground) for f in frames]
    data, _ = st.ComputeBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), road, with_instances=True)
    ref_case = dict(case, segmentation=want_seg)
    for i in range(n):
        ref = helpers.run_oracle(ref_case, image=i)
        assert helpers.sections_equal(ref["sections"], data[i].sections), f"frame {i}"
    # after a compute call the producer leaves the record of the batch alone
    st.GroundTruthOffsetsBatch(1, d_gt.data_ptr(), seg.data_ptr())
    assert st.LastFrames() == n
    assert len(st.InstanceOverlapBatch(n, d_gt.data_ptr())) == n
    # the row end to end: targets into a fresh tensor, ComputeBatch, InstanceOverlapBatch, AP
    fresh = _dev(case["segmentation"])
    row = evaluation.gt_offset_scores(st, cfg.pairwise, big.data_ptr(), fresh.data_ptr(), road, d_gt.data_ptr())
    np.testing.assert_array_equal(fresh.cpu().numpy(), want_seg)
    for i in range(n):
        assert helpers.sections_equal(data[i].sections, row["stixels"][i].sections)
        assert int(row["overlaps"][i]["count"].sum()) == rows * cols
    assert "result" in row and st.LastFrames() == n
    st.close()
