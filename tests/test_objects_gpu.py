"""f9 on the MI355X: is_instance_objects (is_k_objects.hip) and Stixels::InstanceObjectsBatch against the numpy
restatement of tests/objects_reference.py, BYTE for byte: the C ABI on hand-built Sections and maps (tests 1-6 of the
issue), the host class on the output of ComputeBatch with the cluster labels and with the ground-truth vote (test 7).
Canary bytes around every output of the C ABI must survive, and the records behind a capacity keep their fill."""
import numpy as np
import pytest

import assign_gt_reference as ag
import instance_eval_reference as ir
import objects_reference as orf
import render_reference as rr
from instance_stixels_amd import core, host
from instance_stixels_amd.config import SECTION_DTYPE
from test_render_gpu import Out, _dev, _setup, _torch

pytestmark = pytest.mark.gpu

FILL = 0x5C   # Out's body before the call
SPARE = 8     # records behind the capacity that must keep the fill


def _run(secs, inst, rows, cols, object_capacity=None, point_capacity=None):
    """is_instance_objects on host arrays; the capacities default to the restatement's totals.  Returns (objects,
    points, frame_objects, frame_points, totals) with the records cut at the capacities."""
    torch, _ = _torch()
    n, C, S = secs.shape
    want = orf.objects_and_points(secs, inst, rows, cols)
    ocap = len(want[0]) if object_capacity is None else object_capacity
    pcap = len(want[1]) if point_capacity is None else point_capacity
    d_secs = _dev(np.ascontiguousarray(secs).view(np.uint8))
    d_inst = None if inst is None else _dev(np.ascontiguousarray(inst, np.int32))
    objects = Out((ocap + SPARE,), core.OBJECT_DTYPE, fill=FILL)
    points = Out((pcap + SPARE,), core.CONTOUR_DTYPE, fill=FILL)
    fo, fp, totals = Out((n,), np.int32), Out((n,), np.int32), Out((2,), np.int32)
    torch.cuda.synchronize()
    core.instance_objects_ptr(d_sections=d_secs.data_ptr(),
                              d_section_instance=None if inst is None else d_inst.data_ptr(), n_images=n, realcols=C,
                              max_sections=S, rows=rows, cols=cols, object_capacity=ocap, point_capacity=pcap, d_objects=objects.ptr, d_points=points.ptr, d_frame_objects=fo.ptr,
                              d_frame_points=fp.ptr, d_totals=totals.ptr)
    torch.cuda.synchronize()
    o, p = objects.get(), points.get()   # (get() checks the canaries)
    assert (o[ocap:].view(np.uint8) == FILL).all(), "an object was written at or beyond the capacity"
    assert (p[pcap:].view(np.uint8) == FILL).all(), "a point was written at or beyond the capacity"
    return (o[:ocap], p[:pcap], fo.get(), fp.get(), totals.get()), want


def _same(got, want):
    """Bytewise; the restatement's arrays cut where the capacities cut the device's."""
    o, p, fo, fp, totals = got
    wo, wp, wfo, wfp = want
    assert totals.tolist() == [len(wo), len(wp)]
    np.testing.assert_array_equal(fo, wfo)
    np.testing.assert_array_equal(fp, wfp)
    for name in core.OBJECT_DTYPE.names:   # field by field first: a readable message
        np.testing.assert_array_equal(o[name].view(np.int32 if o[name].dtype.itemsize == 4 else np.int64),
                                      wo[name][:len(o)].view(np.int32 if o[name].dtype.itemsize == 4 else np.int64),
                                      err_msg=f"objects.{name}")
    for name in core.CONTOUR_DTYPE.names:
        np.testing.assert_array_equal(p[name].view(np.int32), wp[name][:len(p)].view(np.int32), err_msg=f"points.{name}")
    assert o.tobytes() == wo[:len(o)].tobytes() and p.tobytes() == wp[:len(p)].tobytes()


def _random(n, C, S, rows, seed, labels=6):
    rng = np.random.default_rng(seed)
    secs = np.zeros((n, C, S), SECTION_DTYPE)
    secs["type"] = rng.integers(0, 3, secs.shape)
    secs["vB"] = rng.integers(0, rows, secs.shape)
    secs["vT"] = secs["vB"] + rng.integers(0, rows // 4, secs.shape)
    secs["disparity"] = rng.uniform(0.5, 30, secs.shape)
    secs["semantic_class"] = rng.integers(8, 20, secs.shape)
    secs["type"][rng.random(secs.shape) < 0.08] = -1
    inst = rng.integers(-1, labels, secs.shape).astype(np.int32)
    return secs, inst


def _case_one():
    """The case of the issue's test 1: 3 frames x 70 columns x 8 slots, 64 rows (w = 8)."""
    rows, C, S, n = 64, 70, 8, 3
    secs, inst = _random(n, C, S, rows, seed=1)

    def put(f, c, i, cls, label, d=7.0, vB=10, vT=30):
        secs[f, c, i] = (1, vB, vT, d, cls, 0, 0, 0)
        inst[f, c, i] = label

    secs["type"][0, [5, 10, 20, 21, 22], :] = 2                # (sky, class as drawn, labels as drawn: background)
    secs["type"][0, 60:69, :3] = 2
    put(0, 5, 0, 15, 77)                                       # an instance confined to one column
    for c in range(60, 69):                                    # one over columns 60..68, across the 64-column border
        put(0, c, 1, 13, 9, d=3.0 + c)
    put(0, 10, 2, 12, 9)                                       # the same label under another class
    secs["type"][1, 61, :2] = 2
    put(1, 61, 1, 13, 9)                                       # the same (class, label) in another frame
    put(0, 62, 2, 13, 9, d=90.0, vB=31, vT=40)                 # two members in one column, the second one closer
    put(0, 63, 0, 13, 9, d=66.0, vB=0, vT=9)                   # two with equal disparities: the smaller index
    for i, label in enumerate((-1, 1000, 2**31 - 1)):          # labels that are no instance
        put(0, 20, i, 13, label)
    put(0, 21, 0, 10, 3)                                       # a class-10 and a class-19 section with a label
    put(0, 21, 1, 19, 3)
    secs["type"][0, 22, 2] = -1                                # labelled slots behind a terminator
    for i in range(3, S):
        put(0, 22, i, 13, 500)
    secs["type"][0, 22, 3:] = 1
    for i in range(1, S):                                      # an early terminator in slot 0
        put(2, 0, i, 13, 501)
    secs["type"][2, 0, 0] = -1
    return secs, inst, rows, C * 8


def test_multi_wave_multi_workgroup_case():
    secs, inst, rows, cols = _case_one()
    got, want = _run(secs, inst, rows, cols)
    _same(got, want)
    o, p = got[0], got[1]
    key = lambda f, c, l: o[(o["frame"] == f) & (o["semantic_class"] == c) & (o["label"] == l)]  # noqa: E731
    assert len(key(0, 15, 77)) == 1 and key(0, 15, 77)[0]["n_columns"] == 1
    car = key(0, 13, 9)[0]
    assert car["col_min"] <= 60 and car["col_max"] >= 68 and car["n_columns"] >= 9
    assert len(key(0, 12, 9)) == 1 and len(key(1, 13, 9)) == 1
    mine = p[car["first_point"]:car["first_point"] + car["n_columns"]]
    assert mine[mine["column"] == 62][0]["section"] == 2 and mine[mine["column"] == 62][0]["disparity"] == 90.0
    assert mine[mine["column"] == 63][0]["section"] == 0 and mine[mine["column"] == 63][0]["disparity"] == 66.0
    assert not len(key(0, 13, 500)) and not len(key(2, 13, 501)) and not (o["label"] >= 1000).any()
    assert not np.isin(o["semantic_class"], (10, 19)).any() and (o["reserved"] == 0).all() and (p["reserved"] == 0).all()
    assert got[2].min() > 0 and len(o) > 30, "every frame holds objects"


def test_long_columns():
    """max_sections = 200: 150 members of one instance in column 0 (three rounds of 64), column 1 alternates two
    instances over all 200 slots, without a terminator (then every slot counts); column 2 starts an instance in its
    third round only."""
    rows, C, S = 256, 3, 200
    secs, inst = _random(1, C, S, rows, seed=2)
    secs["type"][secs["type"] == -1] = 1
    secs["semantic_class"][0, :2] = 13
    inst[0, 0] = 1
    secs["type"][0, 0, 150] = -1
    inst[0, 1] = 1 + np.arange(S) % 2
    secs["semantic_class"][0, 2] = 0
    secs["semantic_class"][0, 2, 130:140] = 14
    inst[0, 2] = 3
    got, want = _run(secs, inst, rows, C * 8)
    _same(got, want)
    o = got[0]
    assert [(x["semantic_class"], x["label"], x["n_stixels"]) for x in o] == [(13, 1, 150 + 100), (13, 2, 100), (14, 3, 10)]
    assert o["n_columns"].tolist() == [2, 1, 1] and got[4].tolist() == [3, 4]


def test_clipping_and_odd_values():
    """vB > vT, vT >= rows, negative vB; disparities NaN, +-inf, negative, 40000, +-0: pixels, top / bottom, min / max
    and the Q16 sum agree with the restatement, also for an object of NaNs and one of empty rectangles only."""
    rows, C, S = 64, 4, 12
    secs = np.zeros((1, C, S), SECTION_DTYPE)
    secs["type"] = 1
    secs["semantic_class"] = 13
    inst = np.zeros((1, C, S), np.int32)
    nan2 = np.array(0xFFC00123, np.uint32).view(np.float32)
    odd = [np.nan, np.inf, -np.inf, -3.5, 40000.0, 0.0, -0.0, 32767.998, 32768.0, 1e-7, nan2, 2.5]
    geo = [(40, 10), (10, 200), (-50, 5), (-9, -2), (70, 90), (0, 63), (63, 63), (-2**31, 2**31 - 1), (5, 5), (2**31 - 1, -2**31),
           (20, 30), (31, 20)]
    for c in range(3):
        for i in range(S):
            vB, vT = geo[(i + 5 * c) % S]
            secs[0, c, i] = (1, vB, vT, 0, 13, 0, 0, 0)
        secs["disparity"][0, c] = np.roll(np.array(odd, np.float32), c)
    inst[0, 1, ::2] = 4
    inst[0, 3] = 5                    # column 3: NaNs only
    secs["disparity"][0, 3] = np.nan
    secs["vB"][0, 3], secs["vT"][0, 3] = 10, 20
    secs["semantic_class"][0, 3, 6:] = 14
    secs["vB"][0, 3, 6:], secs["vT"][0, 3, 6:] = 100, 90   # class 14 / label 5: empty rectangles only
    secs["disparity"][0, 3, 8] = np.inf
    got, want = _run(secs, inst, rows, C * 8)
    _same(got, want)
    o = got[0]
    assert [(x["semantic_class"], x["label"]) for x in o] == [(13, 0), (13, 4), (13, 5), (14, 5)]
    assert np.isposinf(o[2]["disparity_min"]) and np.isneginf(o[2]["disparity_max"]) and o[2]["disparity_q16_sum"] == 0
    assert (o[3]["pixels"], o[3]["top"], o[3]["bottom"], o[3]["n_stixels"]) == (0, rows, -1, 6)
    assert np.isneginf(o[0]["disparity_min"]) and np.isposinf(o[0]["disparity_max"])


@pytest.mark.parametrize("C, cols", [(6, 53), (1, 8), (1, 1), (70, 560)])
def test_edge_shapes_and_null_map(C, cols):
    """cols no multiple of realcols, one column, one pixel; a NULL map gives no object and writes no record."""
    rows, S, n = 48, 8, 2
    secs, inst = _random(n, C, S, rows, seed=C + cols, labels=3)
    got, want = _run(secs, inst, rows, cols)
    _same(got, want)
    assert len(got[0]) > 0
    got, want = _run(secs, None, rows, cols, object_capacity=4, point_capacity=4)
    assert got[4].tolist() == [0, 0] and not got[2].any() and not got[3].any() and len(want[0]) == 0
    assert (got[0].view(np.uint8) == FILL).all() and (got[1].view(np.uint8) == FILL).all()


def test_capacities():
    secs, inst, rows, cols = _case_one()
    want = orf.objects_and_points(secs, inst, rows, cols)
    n_objects, n_points = len(want[0]), len(want[1])
    assert n_points > n_objects > 8
    for ocap, pcap in ((n_objects, n_points - 5), (n_objects, 3), (n_objects - 1, n_points), (2, n_points), (0, 0),
                       (1, 1)):
        got, _ = _run(secs, inst, rows, cols, object_capacity=ocap, point_capacity=pcap)
        _same(got, want)    # true totals, the records below the capacities; _run checked the fill behind them


def test_determinism():
    secs, inst, rows, cols = _case_one()
    runs = [_run(secs, inst, rows, cols)[0] for _ in range(3)]
    for r in runs[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(r, runs[0]))


def _host_same(got, secs, maps, rows, cols):
    objects, points, frame_objects, frame_points = got
    want = orf.objects_and_points(secs[:len(frame_objects)], orf.mapping_to_map(maps, secs[:len(maps)].shape), rows, cols)
    _same((objects, points, frame_objects, frame_points, np.array([len(objects), len(points)])), want)
    return want


@pytest.mark.parametrize("preset", ["drn_d_22_unary", "drn_d_38_pairwise"])
def test_host_class_end_to_end(preset):
    """256x512x64, 4 frames (the smallest of test_world_gpu.SHAPES).  The cluster labels of synthetic frames may be
    sparse, so the lower bound on them is one object; the ground-truth vote on instance_eval_reference.synth_gt of the
    same frames must give at least two objects, one over two columns or more -- test_assign_gt_gpu's
    test_host_class_consumers_follow_the_active_map asserts at least 20 labelled stixels for this shape, seed and
    these presets, and the vote labels whole gt instances, which synth_gt draws from multi-column clusters."""
    torch, dev = _torch()
    rows, cols, D, n = 256, 512, 64, 4
    st, case, (big, seg, road), secs, cluster_maps = _setup(preset, rows, cols, D, n, {}, seed=rows + n)
    cfg = case["cfg"]
    got = st.InstanceObjectsBatch(n)
    want = _host_same(got, secs, cluster_maps, rows, cols)
    assert len(got[0]) >= 1, "no object in the batch"
    # a subset of the frames is the prefix; a caller's stream
    sub = st.InstanceObjectsBatch(2)
    assert sub[0].tobytes() == got[0][:got[2][:2].sum()].tobytes() and np.array_equal(sub[2], got[2][:2])
    s = torch.cuda.Stream(device=dev)
    again = st.InstanceObjectsBatch(n, stream=s.cuda_stream)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, got))
    # the ground-truth vote: the active map changes, the objects follow
    gt = ir.synth_gt(rr.render(secs, rows, cols, cluster_maps)[2], seed=cols + n)
    d_gt = _dev(gt)
    torch.cuda.synchronize()
    gt_maps = st.AssignInstancesGTBatch(n, d_gt.data_ptr())
    assert gt_maps == ag.mappings(ag.assign(secs, gt)[0])
    got_gt = st.InstanceObjectsBatch(n)
    _host_same(got_gt, secs, gt_maps, rows, cols)
    assert len(got_gt[0]) >= 2 and (got_gt[0]["n_columns"] >= 2).any()
    # the growth path: a fresh object, capacity 1 -- the same records as with an ample capacity
    st2 = host.Stixels()
    st2.SetConfig(cfg)
    st2.Initialize(max_batch=n)
    st2.SetInstanceObjectCapacity(1)
    st2.ComputeBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), road, with_instances=True)
    st2.AssignInstancesGTBatch(n, d_gt.data_ptr(), with_mapping=False)
    grown = st2.InstanceObjectsBatch(n)
    assert len(got_gt[0]) > n or len(got_gt[1]) > 8 * n, "the case does not overflow a capacity of one object per frame"
    assert all(a.tobytes() == b.tobytes() for a, b in zip(grown, got_gt))
    st2.close()
    # back to the cluster labels; without instances there are no objects
    st.UseClusterInstances()
    back = st.InstanceObjectsBatch(n)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(back, got))
    st.ComputeBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), road, with_instances=False)
    none = st.InstanceObjectsBatch(n)
    assert len(none[0]) == 0 and len(none[1]) == 0 and not none[2].any() and not none[3].any()
    st.close()
    assert len(want[0]) == len(got[0])


def test_view_stays_valid_and_copy_equals_it():
    """The C view (ish_instance_objects_batch leaves the records in the object's pinned buffer) read after other work
    of the process equals the copying form; the records can be fetched once."""
    import ctypes
    rows, cols, D, n = 256, 512, 64, 4
    st, case, _, secs, maps = _setup("drn_d_22_unary", rows, cols, D, n, {}, seed=rows + n)
    first = st.InstanceObjectsBatch(n)
    L = host.lib()
    fo, fp, totals = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(2, np.int32)
    assert L.ish_instance_objects_batch(st._h, n, fo.ctypes.data, fp.ctypes.data, totals.ctypes.data, None) == 0
    _torch()[0].cuda.synchronize()                    # (unrelated work in between: the view is the object's)
    junk = _dev(np.arange(1 << 16, dtype=np.int32)).cpu()
    assert junk[-1] == (1 << 16) - 1
    o, p = np.empty(int(totals[0]), host.OBJECT_DTYPE), np.empty(int(totals[1]), host.CONTOUR_DTYPE)
    assert L.ish_instance_objects_records(st._h, o.ctypes.data, ctypes.c_int64(o.size), p.ctypes.data,
                                          ctypes.c_int64(p.size)) == 0
    assert o.tobytes() == first[0].tobytes() and p.tobytes() == first[1].tobytes()
    assert np.array_equal(fo, first[2]) and np.array_equal(fp, first[3])
    # the view is handed out once; a too small array is refused
    assert L.ish_instance_objects_records(st._h, o.ctypes.data, ctypes.c_int64(o.size), p.ctypes.data,
                                          ctypes.c_int64(p.size)) != 0
    st.close()


def test_host_class_refusals():
    """Parallel to test_world_gpu.test_host_class_refusals: before any compute, n_images outside the last batch."""
    import helpers
    case = helpers.build_case("drn_d_22_unary", 128, 256, 32, seed=3, n_images=2)
    cfg = case["cfg"]
    st = host.Stixels()
    st.SetConfig(cfg)
    st.Initialize(max_batch=2)
    with pytest.raises(ValueError, match="there are none"):
        st.InstanceObjectsBatch(1)
    big, seg = _dev(case["disparity"]), _dev(case["segmentation"])
    road = [(f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground) for f in case["frames"]]
    st.ComputeBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), road[:1])
    for bad in (0, 2):
        with pytest.raises(ValueError, match="n_images outside"):
            st.InstanceObjectsBatch(bad)
    for bad in (0, -5, 10 ** 9):
        with pytest.raises(ValueError, match="SetInstanceObjectCapacity"):
            st.SetInstanceObjectCapacity(bad)
    assert len(st.InstanceObjectsBatch(1)) == 4
    st.close()


def test_objects_are_refused_after_a_gather():
    """ComputeBatchGather leaves this rank's shard in d_stixels: InstanceObjectsBatch refuses it as WorldBatch does (a
    fresh child process with a one-rank RCCL communicator, tests/objects_gather_child.py)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(root, "tests", "objects_gather_child.py")],
                         capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert out.returncode == 0 and "OBJECTS_GATHER_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
