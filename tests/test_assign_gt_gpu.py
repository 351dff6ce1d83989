"""f8 on the MI355X: is_assign_instances_gt (is_k_assign_gt.hip) and Stixels::AssignInstancesGTBatch against the numpy
restatement of tests/assign_gt_reference.py, bit for bit on labels and votes, and through the three consumers
(RenderBatch, InstanceOverlapBatch, WorldBatch) against their own numpy references fed with the restatement's labels.
Canary bytes around every output of the C ABI must survive."""
import numpy as np
import pytest

import assign_gt_reference as ag
import helpers
import instance_eval_reference as ir
import render_reference as rr
import world_reference as wr
from instance_stixels_amd import core, evaluation, host, synthetic
from instance_stixels_amd.config import SECTION_DTYPE
from test_assign_gt_cpu import GOLDEN, fixture_case
from test_render_gpu import PRESETS, Out, _dev, _setup, _torch

pytestmark = pytest.mark.gpu


def _c_abi(secs, gt, votes=True, gt_offset=0, **params):
    """is_assign_instances_gt on host arrays -> (labels, votes) as numpy; gt_offset: bytes the device copy of the
    ground truth is shifted by (a multiple of 4), to leave the 16-byte alignment of the vector path."""
    torch, dev = _torch()
    n, C, S = secs.shape
    _, rows, cols = gt.shape
    d_secs = _dev(np.ascontiguousarray(secs).view(np.uint8))
    raw = torch.zeros(gt.size * 4 + 64, dtype=torch.uint8, device=dev)
    raw[gt_offset:gt_offset + gt.size * 4] = _dev(np.ascontiguousarray(gt, np.int32).view(np.uint8).ravel())
    lab, vot = Out((n, C, S), np.int32), Out((n, C, S), np.int32)
    torch.cuda.synchronize()
    core.assign_instances_gt_ptr(d_sections=d_secs.data_ptr(), d_gt_instance=raw.data_ptr() + gt_offset, n_images=n,
                                 rows=rows, cols=cols, realcols=C, max_sections=S, d_section_instance=lab.ptr,
                                 d_section_votes=vot.ptr if votes else None, **params)
    torch.cuda.synchronize()
    return lab.get(), vot.get() if votes else None


def _same(got, want):
    np.testing.assert_array_equal(got[0], want[0], err_msg="labels")
    if got[1] is not None:
        np.testing.assert_array_equal(got[1], want[1], err_msg="votes")


@pytest.mark.parametrize("k", [0, 1, 2])
def test_c_abi_on_the_fixture_cases(k):
    """The cases of the reference's own Python: through the restatement, the device gives the reference's labels."""
    secs, gt, ref = fixture_case(np.load(GOLDEN), k)
    want = ag.assign(secs[None], gt[None])
    got = _c_abi(secs[None], gt[None])
    _same(got, want)
    cls = secs["semantic_class"]
    np.testing.assert_array_equal(got[0][0], np.where(ref >= 0, ref - cls * 1000, -1))
    assert (got[0] >= 0).sum() >= 50
    _same(_c_abi(secs[None], gt[None], votes=False), want)               # without the optional output
    _same(_c_abi(secs[None], gt[None], gt_offset=4), want)               # a misaligned ground-truth pointer
    for params in (dict(min_fraction=0.5), dict(min_fraction=-1.0), dict(label_ids=[33, 32, 31, 28, 27, 26, 25, 24])):
        _same(_c_abi(secs[None], gt[None], **params), ag.assign(secs[None], gt[None], **params))
    train = np.where(gt >= 24000, gt - (gt // 1000) * 1000 + 13000, gt)  # everything from 24000 up becomes a car
    _same(_c_abi(secs[None], train[None], gt_is_train_ids=1), ag.assign(secs[None], train[None], gt_is_train_ids=True))


def _hand_built(n, rows, C, S, w, tail, seed):
    """Random well-formed columns of random classes and a Cityscapes-like gt with many instances per stixel."""
    rng = np.random.default_rng(seed)
    cols = C * w + tail
    secs = np.zeros((n, C, S), SECTION_DTYPE)
    secs["type"] = -1
    for f in range(n):
        for c in range(C):
            cuts = sorted(rng.choice(np.arange(1, rows), min(S - 2, 5), replace=False).tolist()) + [rows]
            v = 0
            for i, cut in enumerate(cuts):
                secs[f, c, i] = (int(rng.integers(0, 3)), v, cut - 1, 5.0, int(rng.integers(8, 20)), 0, 0, 0)
                v = cut
    lab = np.array([24, 25, 26, 27, 28, 31, 32, 33, 7, 29], np.int32)
    shape = (n, rows // 12 + 1, cols // 6 + 1)                          # blocks of 12 rows x 6 pixels
    blocks = lab[rng.integers(0, 10, shape)] * 1000 + rng.integers(0, 3, shape).astype(np.int32)
    gt = blocks.repeat(12, 1).repeat(6, 2)[:, :rows, :cols].astype(np.int32)
    for f in range(n):                                                  # half of the stixels: mostly their own class
        for c in range(C):
            for i in range(S):
                s = secs[f, c, i]
                if s["type"] == -1:
                    break
                if 11 <= s["semantic_class"] <= 18 and rng.random() < 0.5:
                    own = ag.CITYSCAPES_LABEL_IDS[int(s["semantic_class"]) - 11] * 1000 + int(rng.integers(0, 3))
                    box = gt[f, max(rows - 1 - int(s["vT"]), 0):max(rows - int(s["vB"]), 0), c * w:c * w + w]
                    box[rng.random(box.shape) < 0.7] = own
    return secs, np.ascontiguousarray(gt)


@pytest.mark.parametrize("w, tail", [(4, 0), (8, 0), (16, 0), (8, 5), (9, 3), (1, 0)])
def test_c_abi_widths_and_tails(w, tail):
    """w of 4, 8 and 16, cols % 8 != 0, and hostile ground truth (negative values, >= 34000)."""
    secs, gt = _hand_built(3, 96, 10, 12, w, tail, seed=w * 10 + tail)
    rng = np.random.default_rng(w)
    hostile = rng.random(gt.shape) < 0.05
    gt[hostile] = rng.choice(np.array([-1, -26001, -2**31, 34000, 2**31 - 1, 99999, 1000, 26], np.int32),
                             int(hostile.sum()))
    want = ag.assign(secs, gt)
    assert (want[0] >= 0).sum() >= 10 and (want[1] > 0).sum() > (want[0] >= 0).sum()
    _same(_c_abi(secs, gt), want)
    _same(_c_abi(secs, gt, gt_offset=8), want)


def test_c_abi_sections_outside_the_frame_and_column_ends():
    """Hand-built Sections reaching outside the frame are clipped: the call returns, the canaries around the outputs
    and the memory next to the ground truth stay untouched, and nothing outside the image is read (the restatement
    sees only the image).  Columns without a terminator and with one in slot 0."""
    rows, C, S, w = 64, 9, 70, 8                       # S > 64: two rounds of headers per column
    secs, gt = _hand_built(2, rows, C, S, w, 0, seed=3)
    big = 2**31 - 1
    secs[0, 0, 0] = (1, -big, big, 1.0, 13, 0, 0, 0)
    secs[0, 1, 0] = (1, -5, 10, 1.0, 14, 0, 0, 0)
    secs[0, 2, 1] = (1, rows - 3, rows + 1000, 1.0, 15, 0, 0, 0)
    secs[0, 3, 0] = (1, 40, 20, 1.0, 13, 0, 0, 0)       # vB > vT
    secs[0, 4, 0] = (1, -big - 1, -1, 1.0, 13, 0, 0, 0)  # below the frame altogether
    secs[0, 5, 2] = (1, rows, big, 1.0, 13, 0, 0, 0)     # above it
    secs[1, 0, 0]["type"] = -1                           # a terminator in slot 0 in front of live sections
    for i in range(S):                                   # no terminator: all 70 slots are sections, of 1 or 3 rows
        secs[1, 1, i] = (1, i % rows, min(i % rows + 2 * (i % 2), rows - 1), 1.0, 11 + i % 8, 0, 0, 0)
    for y in range(rows):                                # ... whose bottom row is of their own class
        gt[1, y, w:2 * w] = ag.CITYSCAPES_LABEL_IDS[(rows - 1 - y) % 8] * 1000 + y % 3
    secs[1, 2, 3]["semantic_class"] = -2**31
    secs[1, 2, 4]["semantic_class"] = 2**31 - 1
    want = ag.assign(secs, gt)
    assert (want[0][1, 1] >= 0).sum() > 5 and (want[0][1, 0] == -1).all()
    _same(_c_abi(secs, gt), want)
    _same(_c_abi(secs, gt, gt_offset=12), want)


def test_c_abi_terminator_in_the_second_round_of_headers():
    """Columns of 70 one-row instance-class stixels whose terminator is the 71st entry: the second round of 64 headers
    finds it.  The sections in front of it in that round are voted on; the instance-class sections behind it, over
    rows full of their own class, stay -1 with no vote.  Vector and pixel-by-pixel path."""
    rows, C, S, w, live = 70, 3, 80, 8, 70
    secs = np.zeros((1, C, S), SECTION_DTYPE)
    secs["type"] = -1
    gt = np.zeros((1, rows, C * w), np.int32)
    for y in range(rows):                                # row y is stixel i = rows - 1 - y: its class, number i % 3
        i = rows - 1 - y
        gt[0, y] = ag.CITYSCAPES_LABEL_IDS[i % 8] * 1000 + i % 3
    for c in range(C):
        for i in range(S):
            if i != live:                                # slot 70 stays the terminator
                v = i % rows
                secs[0, c, i] = (1, v, v, 1.0, 11 + v % 8, 0, 0, 0)
    want = ag.assign(secs, gt)
    np.testing.assert_array_equal(want[0][0, :, :live], np.tile(np.arange(live) % 3, (C, 1)))
    assert (want[1][0, :, :live] == w).all()
    assert (want[0][0, :, live:] == -1).all() and (want[1][0, :, live:] == 0).all()
    _same(_c_abi(secs, gt), want)
    _same(_c_abi(secs, gt, gt_offset=4), want)


def _batch(preset, n, k, rows=1024, cols=2048, D=128):
    """A ComputeBatch of n frames of which k are distinct (frame i = frame i % k)."""
    torch, dev = _torch()
    case = helpers.build_case(preset, rows, cols, D, seed=1, n_images=1,
                              size_filter=10 if preset.endswith("unary") else 8)
    cfg = case["cfg"]
    frames = [synthetic.make_frame(cfg, seed=7 + i, n_slabs=12, offset_scale=1.0) for i in range(k)]
    big = torch.from_numpy(np.stack([frames[i % k].disparity for i in range(n)])).to(dev)
    seg = torch.from_numpy(np.stack([frames[i % k].segmentation for i in range(n)])).to(dev)
    road = [(f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground) for f in (frames[i % k] for i in range(n))]
    st = host.Stixels()
    st.SetConfig(cfg)
    st.Initialize(max_batch=n)
    return st, cfg, (big, seg, road)


@pytest.mark.parametrize("preset", PRESETS)
def test_64_frames_full_size_in_both_modes(preset):
    rows, cols, n, k = 1024, 2048, 64, 4
    st, cfg, (big, seg, road) = _batch(preset, n, k)
    data, maps = st.ComputeBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), road, with_instances=True)
    secs = np.stack([d.sections for d in data])
    for i in range(k, n):
        assert secs[i].tobytes() == secs[i % k].tobytes()
    inst = rr.render(secs[:k], rows, cols, maps[:k])[2]
    gt_k = ir.synth_gt(inst, seed=3)
    want_k = ag.assign(secs[:k], gt_k)
    assert (want_k[0] >= 0).sum() >= 50 * k
    gt = np.stack([gt_k[i % k] for i in range(n)])
    want = tuple(np.stack([x[i % k] for i in range(n)]) for x in want_k)
    _same(_c_abi(secs, gt), want)
    # the host class on the same batch: the mapping it returns is the restatement's
    d_gt = _dev(gt)
    _torch()[0].cuda.synchronize()
    got = st.AssignInstancesGTBatch(n, d_gt.data_ptr())
    assert got == ag.mappings(want[0])
    st.close()


def _consumers(st, cfg, n, rows, cols, d_gt):
    """(instance image, overlap tables, world records) of the object's current instance map."""
    img = Out((n, rows, cols), np.int32)
    _torch()[0].cuda.synchronize()
    st.RenderBatch(n, instance=img.ptr)
    tables = st.InstanceOverlapBatch(n, d_gt.data_ptr())
    offsets, records = st.WorldBatch(n)
    return img.get(), tables, (offsets.copy(), records.copy())


def _check_consumers(got, secs, maps, gt, cfg, data):
    img, tables, (offsets, records) = got
    n, rows, cols = img.shape
    inst = rr.render(secs, rows, cols, maps)[2]
    np.testing.assert_array_equal(img, inst)
    for f in range(n):
        np.testing.assert_array_equal(tables[f], ir.joint_histogram(inst[f], gt[f]), err_msg=f"frame {f}")
        wr.assert_records_equal(records[offsets[f]:offsets[f + 1]], wr.records_of(cfg, data[f], maps[f]))
    return inst


@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("with_instances", [True, False])
def test_host_class_consumers_follow_the_active_map(preset, with_instances):
    """After AssignInstancesGTBatch the instance image, the overlap tables and the world's instance_id are those of
    the restatement's labels through the consumers' own references; after UseClusterInstances() or a new compute
    they are the cluster labels' again.  Also after a ComputeBatch WITHOUT instances: the vote needs no candidates."""
    rows, cols, D, n = 256, 512, 64, 4
    st, case, (big, seg, road), secs, cluster_maps = _setup(preset, rows, cols, D, n, {}, seed=rows + n)
    cfg = case["cfg"]
    data, maps = st.ComputeBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), road, with_instances=with_instances)
    assert np.stack([d.sections for d in data]).tobytes() == secs.tobytes()
    gt = ir.synth_gt(rr.render(secs, rows, cols, cluster_maps)[2], seed=cols + n)
    d_gt = _dev(gt)
    before = _consumers(st, cfg, n, rows, cols, d_gt) if with_instances else None
    if with_instances:
        _check_consumers(before, secs, cluster_maps, gt, cfg, data)
    else:
        with pytest.raises(ValueError, match="instances"):
            st.InstanceOverlapBatch(n, d_gt.data_ptr())

    want_labels = ag.assign(secs, gt)[0]
    want_maps = ag.mappings(want_labels)
    assert sum(len(m) for m in want_maps) >= 20, "the case labels nothing"
    assert want_maps != cluster_maps
    assert st.AssignInstancesGTBatch(n, d_gt.data_ptr()) == want_maps
    inst = _check_consumers(_consumers(st, cfg, n, rows, cols, d_gt), secs, want_maps, gt, cfg, data)
    # the AP of the batch through the table-based evaluator equals the per-mask evaluation of the same labels
    ev = evaluation.CityscapesInstanceEval()
    ev.add(st.InstanceOverlapBatch(n, d_gt.data_ptr()))
    np.testing.assert_allclose(ev.result()["ap"], ir.masks_ap(list(zip(inst, gt))), rtol=0, atol=1e-12)
    # a vote over fewer frames: the others have no instances; without the mapping nothing comes back
    assert st.AssignInstancesGTBatch(2, d_gt.data_ptr(), with_mapping=False) is None
    _check_consumers(_consumers(st, cfg, n, rows, cols, d_gt), secs, want_maps[:2] + [{}] * (n - 2), gt, cfg, data)
    # other parameters reach the kernel
    st.SetGTAssignmentParameters(0.6)
    assert st.AssignInstancesGTBatch(n, d_gt.data_ptr()) == ag.mappings(ag.assign(secs, gt, min_fraction=0.6)[0])
    st.SetGTAssignmentParameters()
    with pytest.raises(ValueError, match="n_images"):
        st.AssignInstancesGTBatch(n + 1, d_gt.data_ptr())

    st.UseClusterInstances()
    if with_instances:
        after = _consumers(st, cfg, n, rows, cols, d_gt)
        assert after[0].tobytes() == before[0].tobytes() and after[2][1].tobytes() == before[2][1].tobytes()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(after[1], before[1]))
    else:
        with pytest.raises(ValueError, match="instances"):
            st.RenderBatch(n, instance=Out((n, rows, cols), np.int32).ptr)
        assert (st.WorldBatch(n)[1]["instance_id"] == -1).all()
    # a new compute call ends the ground-truth map too
    st.AssignInstancesGTBatch(n, d_gt.data_ptr())
    st.ComputeBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), road, with_instances=True)
    _check_consumers(_consumers(st, cfg, n, rows, cols, d_gt), secs, cluster_maps, gt, cfg, data)
    st.close()


@pytest.mark.parametrize("preset", PRESETS)
def test_after_compute_single_frame(preset):
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
    secs = data.sections[None]
    cluster = st.GetInstanceStixels()
    gt = ir.synth_gt(rr.render(secs, rows, cols, [cluster])[2], seed=9)
    d_gt = _dev(gt)
    want = ag.mappings(ag.assign(secs, gt)[0])
    assert len(want[0]) >= 10
    assert st.AssignInstancesGTBatch(1, d_gt.data_ptr()) == want
    _check_consumers(_consumers(st, cfg, 1, rows, cols, d_gt), secs, want, gt, cfg, [data])
    st.Compute(cfg.pairwise)
    _check_consumers(_consumers(st, cfg, 1, rows, cols, d_gt), secs, [cluster], gt, cfg, [data])
    st.close()


def test_pack_section_labels_c_abi():
    """The quads of a hand-made map, as a set; the true count also beyond the capacity; canaries."""
    rng = np.random.default_rng(2)
    n, C, S = 3, 7, 11
    smap = rng.integers(-1, 4, (n, C, S)).astype(np.int32)
    smap[rng.random(smap.shape) < 0.6] = -1
    want = sorted((f, c, s, int(smap[f, c, s])) for f, c, s in zip(*np.nonzero(smap >= 0)))
    d_map = _dev(smap)
    for cap in (len(want) + 5, len(want), 3):
        out = Out((4 + 4 * cap,), np.int32)
        _torch()[0].cuda.synchronize()
        core.pack_section_labels_ptr(d_map.data_ptr(), n, C, S, cap, out.ptr)
        _torch()[0].cuda.synchronize()
        got = out.get()
        assert got[:4].tolist() == [len(want), 0, 0, 0]
        quads = sorted(map(tuple, got[4:4 + 4 * min(cap, len(want))].reshape(-1, 4).tolist()))
        assert quads == want if cap >= len(want) else set(quads) <= set(want) and len(set(quads)) == cap
