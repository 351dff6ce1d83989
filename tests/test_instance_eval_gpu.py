"""f6 on the MI355X: Stixels::InstanceOverlapBatch / is_instance_overlap (is_k_instance_eval.hip) against the numpy
joint histogram of render_reference.render's instance image (tests/instance_eval_reference.py), record for record,
with a Cityscapes-like gt synthesized from that image.  Canaries around every output must survive."""
import numpy as np
import pytest

import helpers
import instance_eval_reference as ir
import render_reference as rr
from instance_stixels_amd import core, evaluation, host, synthetic
from instance_stixels_amd.config import SECTION_DTYPE
from test_render_gpu import PRESETS, SHAPES, Out, _dev, _full, _setup, _torch
from test_road_batch_gpu import _batch, _init

pytestmark = pytest.mark.gpu


def _want(inst, gt):
    return [ir.joint_histogram(i, g) for i, g in zip(inst, gt)]


def _same(got, want, rows, cols):
    assert len(got) == len(want)
    for f, (a, b) in enumerate(zip(got, want)):
        assert int(a["count"].sum()) == rows * cols, f"frame {f}: the table does not sum to rows*cols"
        assert a.dtype == core.OVERLAP_DTYPE
        np.testing.assert_array_equal(a, b, err_msg=f"frame {f}")


@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("rows, cols, D, n, ov", SHAPES)
def test_overlap_batch_matches_restatement(preset, rows, cols, D, n, ov):
    st, case, _, secs, maps = _setup(preset, rows, cols, D, n, ov, seed=rows + n)
    inst = rr.render(secs, rows, cols, maps)[2]
    gt = ir.synth_gt(inst, seed=cols + n)
    d_gt = _dev(gt)
    _torch()[0].cuda.synchronize()
    got = st.InstanceOverlapBatch(n, d_gt.data_ptr())
    want = _want(inst, gt)
    _same(got, want, rows, cols)
    if rows >= 256:
        assert any((t["pred"] != 0).any() for t in want), "no instance pixels: the case exercises nothing"
    _same(st.InstanceOverlapBatch(1, d_gt.data_ptr()), want[:1], rows, cols)
    # AP from the device tables equals AP from the numpy path, and the tables give the per-mask evaluation
    a, b = evaluation.CityscapesInstanceEval(), evaluation.CityscapesInstanceEval()
    a.add(got)
    b.add(want)
    ra, rb = a.result(), b.result()
    np.testing.assert_array_equal(ra["ap"], rb["ap"])
    if rows <= 256:
        np.testing.assert_allclose(ra["ap"], ir.masks_ap(list(zip(inst, gt))), rtol=0, atol=1e-12)
    st.close()


@pytest.mark.parametrize("preset", PRESETS)
def test_overlap_after_compute_single_frame(preset):
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
    inst = rr.render(data.sections[None], rows, cols, [st.GetInstanceStixels()])[2]
    assert (inst != 0).any()
    gt = ir.synth_gt(inst, seed=9)
    d_gt = _dev(gt)
    _same(st.InstanceOverlapBatch(1, d_gt.data_ptr()), _want(inst, gt), rows, cols)
    with pytest.raises(ValueError, match="n_images"):
        st.InstanceOverlapBatch(2, d_gt.data_ptr())
    st.close()


def test_overlap_64_frames_full_size():
    rows, cols, D, n = 1024, 2048, 128, 64
    case = helpers.build_case("drn_d_22_unary", rows, cols, D, seed=1, n_images=8, size_filter=10)
    torch, dev = _torch()
    k = len(case["frames"])
    frames = [synthetic.make_frame(case["cfg"], seed=7 + i, n_slabs=12, offset_scale=1.0) for i in range(k)]
    big = torch.from_numpy(np.stack([frames[i % k].disparity for i in range(n)])).to(dev)
    seg = torch.from_numpy(np.stack([frames[i % k].segmentation for i in range(n)])).to(dev)
    road = [(f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground) for f in (frames[i % k] for i in range(n))]
    st = host.Stixels()
    st.SetConfig(case["cfg"])
    st.Initialize(max_batch=n)
    data, maps = st.ComputeBatch(case["cfg"].pairwise, big.data_ptr(), seg.data_ptr(), road, with_instances=True)
    secs = np.stack([d.sections for d in data])
    # the numpy path on 8 distinct frames, the gt of frame i is that of frame i % 8 (its Sections are the same)
    inst8 = rr.render(secs[:k], rows, cols, maps[:k])[2]
    gt8 = ir.synth_gt(inst8, seed=3)
    d_gt = _dev(np.stack([gt8[i % k] for i in range(n)]))
    want8 = _want(inst8, gt8)
    got = st.InstanceOverlapBatch(n, d_gt.data_ptr())
    _same(got, [want8[i % k] for i in range(n)], rows, cols)
    again = st.InstanceOverlapBatch(n, d_gt.data_ptr())
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    st.close()


def test_overlap_streams_canaries_determinism_overflow_and_refusals():
    torch, dev = _torch()
    rows, cols, D, n = 256, 512, 64, 4
    st, case, (big, seg, road), secs, maps = _setup("drn_d_38_pairwise", rows, cols, D, n, {}, seed=3)
    inst = rr.render(secs, rows, cols, maps)[2]
    gt = ir.synth_gt(inst, seed=4)
    d_gt = _dev(gt)
    want = _want(inst, gt)
    base = st.InstanceOverlapBatch(n, d_gt.data_ptr())
    _same(base, want, rows, cols)
    stream = torch.cuda.Stream(device=dev)
    _same(st.InstanceOverlapBatch(n, d_gt.data_ptr(), stream=stream.cuda_stream), want, rows, cols)
    # forced overflow in the host class: every frame is repeated alone, the tables stay complete
    st.SetInstanceOverlapCapacity(3)
    _same(st.InstanceOverlapBatch(n, d_gt.data_ptr()), want, rows, cols)
    st.SetInstanceOverlapCapacity(4096)
    # hostile gt (a new value per pixel) in frame 1: its table has rows*cols records, still complete
    hostile = gt.copy()
    hostile[1] = np.random.default_rng(0).integers(-2**31, 2**31 - 1, (rows, cols), dtype=np.int64).astype(np.int32)
    d_h = _dev(hostile)
    wh = _want(inst, hostile)
    _same(st.InstanceOverlapBatch(n, d_h.data_ptr()), wh, rows, cols)
    # refusals under the RenderBatch rules
    with pytest.raises(ValueError, match="n_images"):
        st.InstanceOverlapBatch(n + 1, d_gt.data_ptr())
    st.ComputeBatch(True, big.data_ptr(), seg.data_ptr(), road[:2], with_instances=False)
    with pytest.raises(ValueError, match="instances"):
        st.InstanceOverlapBatch(2, d_gt.data_ptr())
    st.close()


def test_finish_then_initialize_again_matches_a_fresh_object():
    """Finish() releases every buffer the calls grew; InitializeBatch with another batch size on the same object then
    gives what a fresh object gives, bit for bit: ComputeBatch with instances, RenderBatch, InstanceOverlapBatch
    through its overflow retries, and RoadEstimation::ComputeBatch."""
    rows, cols, D, n = 256, 512, 64, 4
    st, case, (big, seg, road), _, _ = _setup("drn_d_38_pairwise", rows, cols, D, n, {}, seed=rows + n)
    cfg = case["cfg"]
    rng = np.random.default_rng(12)
    gt = rng.integers(0, 40, (n, rows, cols)).astype(np.uint8)
    gd = rng.uniform(0, 50, (n, rows, cols)).astype(np.float32)
    d_gi = _dev(rng.integers(0, 6, (n, rows, cols)).astype(np.int32))

    def run(obj, m):
        data, maps = obj.ComputeBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), road[:m], with_instances=True)
        assert any(maps), "no instances: the case does not exercise the instance buffers"
        rendered = _full(obj, m, (m, rows, cols), gt[:m], gd[:m])
        obj.SetInstanceOverlapCapacity(3)  # every frame overflows it: the retries with larger tables run
        tables = obj.InstanceOverlapBatch(m, d_gi.data_ptr())
        assert all(len(t) > 3 for t in tables)
        return ([d.sections.tobytes() for d in data], maps, [np.asarray(x).tobytes() for x in rendered],
                [t.tobytes() for t in tables])

    for m in (n, 2, 3):  # the same object: Initialize(n) by _setup, then Finish -> Initialize(m)
        if m != n:
            st.Finish()
            st.Initialize(max_batch=m)
        fresh = host.Stixels()
        fresh.SetConfig(cfg)
        fresh.Initialize(max_batch=m)
        assert run(st, m) == run(fresh, m), m
        fresh.close()
    st.close()

    disp, cases = _batch(rows, cols, D, n, seed=13)
    d = _torch()[0].from_numpy(disp).to(_torch()[1])
    re_ = host.RoadEstimation()
    _init(re_, cases[0]["cfg"], rows, cols, D)
    for m in (n, 2):
        if m != n:
            re_.Finish()
            _init(re_, cases[0]["cfg"], rows, cols, D)
        fresh = host.RoadEstimation()
        _init(fresh, cases[0]["cfg"], rows, cols, D)
        got, want = re_.ComputeBatch(d.data_ptr(), m), fresh.ComputeBatch(d.data_ptr(), m)
        assert got == want and any(got[1]), m
        fresh.close()
    re_.close()


def _c_abi(secs_dev, map_dev, n, realcols, S, rows, cols, d_gt, cap, offset=0):
    rec = Out((n, cap), core.OVERLAP_DTYPE, offset=offset)
    nrec, ovf = Out((n,), np.int32), Out((n,), np.int32)
    torch = _torch()[0]
    torch.cuda.synchronize()
    core.instance_overlap_ptr(d_sections=secs_dev, d_section_instance=map_dev, n_images=n, realcols=realcols,
                              max_sections=S, rows=rows, cols=cols, d_gt_instance=d_gt, capacity=cap,
                              d_records=rec.ptr, d_n_records=nrec.ptr, d_overflow=ovf.ptr)
    torch.cuda.synchronize()
    return rec.get(), nrec.get(), ovf.get()


def test_c_abi_overflow_flags_exactly_the_frames_and_stays_in_bounds():
    """is_instance_overlap straight from hand-made per-section maps: frames with more distinct pairs than the
    capacity are flagged (hostile gt included), the others exact; canaries around records, counts and flags."""
    rows, realcols, cols, S = 128, 16, 133, 8        # w = 8, a 5-pixel tail, the per-pixel path
    rng = np.random.default_rng(5)
    n = 3
    secs = np.zeros((n, realcols, S), SECTION_DTYPE)
    secs["type"] = -1
    smap = np.full((n, realcols, S), -1, np.int32)
    for f in range(n):
        for c in range(realcols):
            cuts = sorted(rng.choice(np.arange(1, rows), 3, replace=False).tolist()) + [rows]
            v = 0
            for k, cut in enumerate(cuts):
                secs[f, c, k] = (1, v, cut - 1, 5.0, int(rng.integers(11, 19)), 0, 0, 0)
                smap[f, c, k] = int(rng.integers(-1, 3))
                v = cut
            secs[f, c, len(cuts)]["type"] = -1
    # the one pair the hash cannot hold as a key (pred = gt = INT32_MAX): class 152471339 * 1000 + 7 wraps to it
    secs[0, 1, 0]["semantic_class"] = 152471339
    smap[0, 1, 0] = 7
    maps = [{(c, k): int(smap[f, c, k]) for c in range(realcols) for k in range(S) if smap[f, c, k] >= 0}
            for f in range(n)]
    inst = rr.render(secs, rows, cols, maps)[2]
    gt = ir.synth_gt(inst, seed=11)
    gt[0, rows - int(secs[0, 1, 0]["vT"]) - 1:, 8:16] = 2**31 - 1
    gt[2] = rng.integers(-2**31, 2**31 - 1, (rows, cols), dtype=np.int64).astype(np.int32)   # hostile
    want = _want(inst, gt)
    sizes = [len(t) for t in want]
    assert want[0][-1]["pred"] == want[0][-1]["gt"] == 2**31 - 1
    cap = max(sizes[0], sizes[1]) + 1
    assert sizes[2] > cap
    d_secs, d_map, d_gt = _dev(secs.view(np.uint8)), _dev(smap), _dev(gt)
    rec, nrec, ovf = _c_abi(d_secs.data_ptr(), d_map.data_ptr(), n, realcols, S, rows, cols, d_gt.data_ptr(), cap,
                            offset=8)
    assert ovf.tolist() == [0, 0, 1] and nrec.tolist() == [sizes[0], sizes[1], 0]
    for f in range(2):
        np.testing.assert_array_equal(rec[f, :sizes[f]], want[f])
    # a capacity of exactly a frame's size fits it; one less overflows it
    rec, nrec, ovf = _c_abi(d_secs.data_ptr(), d_map.data_ptr(), 1, realcols, S, rows, cols, d_gt.data_ptr(),
                            sizes[0])
    assert ovf.tolist() == [0] and nrec.tolist() == [sizes[0]]
    np.testing.assert_array_equal(rec[0], want[0])
    rec, nrec, ovf = _c_abi(d_secs.data_ptr(), d_map.data_ptr(), 1, realcols, S, rows, cols, d_gt.data_ptr(),
                            sizes[0] - 1)
    assert ovf.tolist() == [1] and nrec.tolist() == [0]
    # rows*cols always fits, hostile gt included; two runs give the same bytes
    r1 = _c_abi(d_secs.data_ptr(), d_map.data_ptr(), n, realcols, S, rows, cols, d_gt.data_ptr(), rows * cols)
    r2 = _c_abi(d_secs.data_ptr(), d_map.data_ptr(), n, realcols, S, rows, cols, d_gt.data_ptr(), rows * cols)
    assert r1[2].tolist() == [0, 0, 0] and r1[1].tolist() == sizes
    for f in range(n):
        np.testing.assert_array_equal(r1[0][f, :sizes[f]], want[f])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(r1, r2))
    # no map: every pixel is pred 0
    r0 = _c_abi(d_secs.data_ptr(), None, 2, realcols, S, rows, cols, d_gt.data_ptr(), rows * cols)
    for f in range(2):
        np.testing.assert_array_equal(r0[0][f, :r0[1][f]], ir.joint_histogram(np.zeros_like(inst[f]), gt[f]))
