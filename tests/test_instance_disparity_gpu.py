"""f10 on the MI355X: is_cluster_instance_disparity (is_k_instance_disparity.hip) and
Stixels::ClusterInstanceDisparityBatch against the numpy restatement (tests/instance_disparity_reference.py), which
tests/test_instance_disparity_cpu.py pins on the reference's own Python.  Everything is exact: the key counts and
medians, the stixel medians bit for bit, every label, core-candidate flag and packed triple, the mappings.  The
C-ABI cases start from poisoned outputs and a scratch full of garbage, so nothing they read was left by a call."""
import os

import numpy as np
import pytest

import helpers
import instance_disparity_reference as idr
import instance_eval_reference as ir
import render_reference as rr
from instance_stixels_amd import core as core_mod
from instance_stixels_amd import host, make_config
from instance_stixels_amd.config import SECTION_DTYPE
from oracle import oracle
from test_instance_disparity_cpu import BANDED, banded_frame, class_labels

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_python_disp", "instance_disparity_reference_python.npz")
LABEL_IDS = idr.CITYSCAPES_LABEL_IDS
POISON_LABEL, POISON_FLAG, POISON_PACKED = -7, 9, -9
_CACHE = {}


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _dev(a):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- inputs -------------------------------------------------------------------------------------------------------
def fixture_case(k):
    if ("fixture", k) not in _CACHE:
        g = np.load(GOLDEN)
        raw = g[f"c{k}_sections"]
        meta = g[f"c{k}_meta"]
        _CACHE["fixture", k] = dict(
            sections=np.ascontiguousarray(raw).view(SECTION_DTYPE).reshape(raw.shape[:2])[None],
            gt=g[f"c{k}_gt"].astype(np.int32)[None], disparity_u8=g[f"c{k}_disparity_u8"][None],
            eps=float(g[f"c{k}_eps"]), size_filter=int(meta[5]), min_pts=int(meta[6]))
    return _CACHE["fixture", k]


def make_sections(n, C, S, rows, w, seed, inst_class=None, p_inst=0.5, centres=6):
    """Constructed Sections (no DP): every column cut into 1 .. S-1 stixels, about p_inst of them objects of an
    instance class whose means scatter around a few centres per frame."""
    rng = np.random.default_rng(seed)
    secs = np.zeros((n, C, S), SECTION_DTYPE)
    secs["type"] = -1
    for f in range(n):
        cx = rng.uniform(0, C * w, centres)
        cy = rng.uniform(0, rows, centres)
        for c in range(C):
            k = int(rng.integers(1, S))
            cuts = np.sort(rng.choice(np.arange(1, rows), size=min(k, rows - 1) - 1, replace=False)) if k > 1 else []
            bounds = [0] + [int(v) for v in cuts] + [rows]
            for i in range(len(bounds) - 1):
                inst = rng.random() < p_inst
                cls = (inst_class or int(rng.integers(11, 19))) if inst else int(rng.integers(0, 11))
                j = int(rng.integers(0, centres))
                secs[f, c, i] = (1 if inst else int(rng.integers(0, 3)), bounds[i], bounds[i + 1] - 1,
                                 float(rng.integers(1, 30)), cls, 0.0,
                                 np.float32(cx[j] + rng.normal(0, 6)), np.float32(cy[j] + rng.normal(0, 6)))
    return secs


def make_images(n, rows, cols, seed, n_rects=14, numbers=6):
    """A ground truth of stuff, instance rectangles and hostile values, and a blocky 8-bit disparity with holes."""
    rng = np.random.default_rng(seed)
    gt = np.full((n, rows, cols), 7, np.int32)
    for f in range(n):
        for _ in range(n_rects):
            y, x = int(rng.integers(0, rows)), int(rng.integers(0, cols))
            h, wd = int(rng.integers(2, max(3, rows // 2))), int(rng.integers(2, max(3, cols // 3)))
            gt[f, y:y + h, x:x + wd] = int(rng.choice(LABEL_IDS)) * 1000 + int(rng.integers(0, numbers))
        hostile = rng.random((rows, cols)) < 0.003
        gt[f][hostile] = rng.choice(np.array([-1, -26001, -2**31, 34000, 2**31 - 1, 29003, 1000, 23999], np.int32),
                                    int(hostile.sum()))
    blocks = rng.integers(1, 250, (n, rows // 4 + 1, cols // 4 + 1)).repeat(4, 1).repeat(4, 2)[:, :rows, :cols]
    disp = (blocks + rng.integers(0, 6, (n, rows, cols))).astype(np.uint8)
    disp[rng.random(disp.shape) < 0.05] = 0
    return gt, disp


# ---- the C ABI ----------------------------------------------------------------------------------------------------
class CoreCall:
    """The device arrays of one batch: candidates as k_compact_instances lays them out, poisoned outputs."""

    def __init__(self, sections, gt, disparity_u8, capacity, gt_offset_bytes=0, disp_offset_bytes=0):
        torch, dev = _torch()
        self.n, self.C, self.S = sections.shape
        self.rows, self.cols = gt.shape[1:]
        self.capacity = capacity
        n, slots = self.n, self.C * self.S
        com = np.zeros((n, 8, slots, 2), np.float32)
        idx = np.zeros((n, 8, slots, 2), np.int32)
        per = np.zeros((n, 8), np.int32)
        for f in range(n):
            for cls in range(8):
                ci = idr.candidates(sections[f], cls)
                per[f, cls] = len(ci)
                idx[f, cls, :len(ci)] = ci
                sec = sections[f][ci[:, 0], ci[:, 1]]
                com[f, cls, :len(ci), 0], com[f, cls, :len(ci), 1] = sec["instance_meanx"], sec["instance_meany"]
        self.per = per
        self.d_sections = _dev(sections.view(np.int32).reshape(n, self.C, self.S, 8))
        flat_gt = torch.zeros(gt.size + 4, dtype=torch.int32, device=dev)
        self.gt_view = flat_gt[gt_offset_bytes // 4: gt_offset_bytes // 4 + gt.size]
        self.gt_view.copy_(_dev(gt).reshape(-1))
        flat_d = torch.zeros(disparity_u8.size + 16, dtype=torch.uint8, device=dev)
        self.d_view = flat_d[disp_offset_bytes: disp_offset_bytes + disparity_u8.size]
        self.d_view.copy_(_dev(disparity_u8).reshape(-1))
        self.com, self.idx, self.d_per = _dev(com), _dev(idx), _dev(per)
        self.cand = torch.full((n, 8, slots), POISON_FLAG, dtype=torch.uint8, device=dev)
        self.labels = torch.full((n, 8, slots), POISON_LABEL, dtype=torch.int32, device=dev)
        self.packed = torch.full((n, 1 + 3 * 8 * slots), POISON_PACKED, dtype=torch.int32, device=dev)
        self.bytes = core_mod.instance_disparity_scratch_bytes(n, self.C, self.S, capacity)
        assert self.bytes > 0
        self.scratch = torch.full((self.bytes + 64,), 0xAB, dtype=torch.uint8, device=dev)
        self.key_count = torch.full((n + 1,), -5, dtype=torch.int32, device=dev)
        self.key_median = torch.full((n * idr.KEYS + 1,), 0x7777, dtype=torch.int16, device=dev)
        self.stixel = torch.full((n * slots + 1,), -3.0, dtype=torch.float32, device=dev)

    def run(self, eps, min_pts, size_filter, outputs=True):
        torch, dev = _torch()
        ibs = [core_mod.InstanceBuffers(self.com[f].data_ptr(), self.idx[f].data_ptr(), self.cand[f].data_ptr(),
                                        self.d_per[f].data_ptr(), self.labels[f].data_ptr(), self.packed[f].data_ptr())
               for f in range(self.n)]
        out = dict(d_stixel_median=self.stixel.data_ptr(), d_key_count=self.key_count.data_ptr(),
                   d_key_median=self.key_median.data_ptr()) if outputs else {}
        rc = core_mod.cluster_instance_disparity_ptr(
            ibs, stream=torch.cuda.current_stream(dev).cuda_stream, d_sections=self.d_sections.data_ptr(),
            d_gt_instance=self.gt_view.data_ptr(), d_disparity_u8=self.d_view.data_ptr(), n_images=self.n,
            rows=self.rows, cols=self.cols, realcols=self.C, max_sections=self.S, eps=eps, min_pts=min_pts,
            size_filter=size_filter, capacity=self.capacity, d_scratch=self.scratch.data_ptr(),
            scratch_bytes=self.bytes, **out)
        assert rc == 0, core_mod.lib().is_last_error().decode()
        torch.cuda.synchronize(dev)
        # nothing behind the scratch and the optional outputs was written
        assert (self.scratch[self.bytes:] == 0xAB).all()
        assert int(self.key_count[-1]) == -5 and int(self.key_median[-1]) == 0x7777 and float(self.stixel[-1]) == -3.0
        return self

    def check(self, want, outputs=True):
        n, slots = self.n, self.C * self.S
        if outputs:
            np.testing.assert_array_equal(self.key_count[:n].cpu().numpy(), want["key_count"])
            np.testing.assert_array_equal(self.key_median[:-1].cpu().numpy().view(np.uint16).reshape(n, idr.KEYS),
                                          want["key_median"])
            got = self.stixel[:-1].cpu().numpy().reshape(n, self.C, self.S)
            np.testing.assert_array_equal(got.view(np.uint32), want["stixel_median"].view(np.uint32))
        labels, cand, packed = self.labels.cpu().numpy(), self.cand.cpu().numpy(), self.packed.cpu().numpy()
        for f in range(n):
            for cls, (idx, lab, large) in enumerate(want["per_class"][f]):
                m = len(idx)
                np.testing.assert_array_equal(labels[f, cls, :m], lab, err_msg=f"labels of frame {f} class {11 + cls}")
                np.testing.assert_array_equal(cand[f, cls, :m], large, err_msg=f"flags of frame {f} class {11 + cls}")
                assert (labels[f, cls, m:] == POISON_LABEL).all() and (cand[f, cls, m:] == POISON_FLAG).all()
            tri = want["packed"][f]
            assert packed[f, 0] == len(tri)
            np.testing.assert_array_equal(packed[f, 1:1 + 3 * len(tri)].reshape(-1, 3), tri)
            assert (packed[f, 1 + 3 * len(tri):] == POISON_PACKED).all()

    def untouched(self):
        return bool((self.labels == POISON_LABEL).all() and (self.cand == POISON_FLAG).all() and
                    (self.packed == POISON_PACKED).all())


def _core_case(sections, gt, disp, eps, min_pts, size_filter, capacity=64, **kw):
    want = idr.run(sections, gt, disp, eps, min_pts, size_filter)
    assert max(want["key_count"]) <= capacity
    call = CoreCall(sections, gt, disp, capacity, **kw).run(eps, min_pts, size_filter)
    call.check(want)
    return call, want


@pytest.mark.parametrize("k", [0, 1, 2])
def test_fixture_cases(k):
    c = fixture_case(k)
    call, want = _core_case(c["sections"], c["gt"], c["disparity_u8"], c["eps"], c["min_pts"], c["size_filter"])
    assert (want["label_map"] >= 0).any() and (want["stixel_median"] * 4 % 2 == 1).any()
    # a second call with another eps on the same arrays and scratch equals a fresh one: no state is left
    other = idr.run(c["sections"], c["gt"], c["disparity_u8"], c["eps"] * 0.5, c["min_pts"], c["size_filter"])
    assert any(not np.array_equal(a[1], b[1]) for a, b in zip(other["per_class"][0], want["per_class"][0]))
    call.run(c["eps"] * 0.5, c["min_pts"], c["size_filter"]).check(other)
    # ... and without the optional outputs the labels are the same
    call.run(c["eps"], c["min_pts"], c["size_filter"], outputs=False).check(want, outputs=False)


def test_three_distinct_frames():
    """Frame 0 as it stands, frame 1 without an instance pixel, frame 2 without an instance-class stixel."""
    c = fixture_case(2)
    rows, cols = c["gt"].shape[1:]
    C, S = c["sections"].shape[1:]
    secs = np.concatenate([c["sections"], make_sections(1, C, S, rows, cols // C, seed=4), c["sections"]])
    inst = (secs[2]["semantic_class"] >= 11) & (secs[2]["type"] != -1)
    secs[2]["semantic_class"][inst] = 3
    gt2, d2 = make_images(2, rows, cols, seed=5)
    gt = np.concatenate([c["gt"], np.full_like(c["gt"], 7), gt2[:1]])
    gt[1, ::3, ::5] = 23005                                   # stuff with an id > 1000 is no instance either
    disp = np.concatenate([c["disparity_u8"], d2])
    call, want = _core_case(secs, gt, disp, c["eps"], c["min_pts"], c["size_filter"])
    assert want["key_count"][1] == 0 and want["key_count"][0] > 0 and want["key_count"][2] > 0
    assert len(want["packed"][2]) == 0 and len(want["packed"][1]) > 0 and not want["stixel_median"][1].any()
    assert (want["label_map"][0] >= 0).any()


@pytest.mark.parametrize("cols, C, gt_off, d_off", [
    (44, 5, 0, 0),     # cols % 8 == 4: pixel by pixel, a last row piece of four pixels
    (40, 5, 0, 0),     # vector loads; 5 stixel columns: the second workgroup of four waves is partly empty
    (40, 5, 4, 0),     # the ground truth 4 bytes off a 16-byte boundary: the scalar path
    (40, 5, 0, 3),     # the disparity off its 8-byte boundary
    (72, 12, 0, 0),    # w = 6
])
def test_odd_shapes_and_alignments(cols, C, gt_off, d_off):
    rows, S = 37, 9
    secs = make_sections(2, C, S, rows, cols // C, seed=cols + gt_off + d_off, inst_class=13, p_inst=0.7, centres=2)
    gt, disp = make_images(2, rows, cols, seed=cols)
    _, want = _core_case(secs, gt, disp, 14.0, 2, 3, gt_offset_bytes=gt_off, disp_offset_bytes=d_off)
    assert (want["stixel_median"] != 0).any() and (want["label_map"] >= 0).any()


def test_one_key_over_the_whole_image():
    rows, cols, C, S = 64, 256, 32, 6
    secs = make_sections(1, C, S, rows, 8, seed=8)
    _, disp = make_images(1, rows, cols, seed=8)
    gt = np.full((1, rows, cols), 26001, np.int32)
    _, want = _core_case(secs, gt, disp, 20.0, 2, 3, capacity=1)
    assert want["key_count"].tolist() == [1]
    med = want["stixel_median"][0]
    assert set(np.unique(med).tolist()) == {0.0, float(want["key_median"][0, 2001]) * 0.5}


def test_a_stixel_of_height_one_and_one_of_full_height():
    rows, cols, C, S = 70, 32, 4, 72
    secs = np.zeros((1, C, S), SECTION_DTYPE)
    secs["type"] = -1
    secs[0, 0, 0] = (1, 0, rows - 1, 5.0, 13, 0, 4.0, 30.0)                  # more rows than a wave has lanes
    for i in range(rows):                                                     # 70 stixels: two rounds of headers
        secs[0, 1, i] = (1, i, i, 5.0, 13 if i % 2 else 12, 0, 12.0, float(i))
    secs[0, 2, 0] = (1, 0, 0, 5.0, 18, 0, 20.0, 0.0)
    secs[0, 2, 1] = (1, 1, rows - 1, 5.0, 18, 0, 20.0, 35.0)
    # behind the terminators (slot 70 of column 1: found in the second round; slot 2 of column 2): full-height sections
    # of an instance class, which are no stixels -- median 0, no candidate
    secs[0, 1, 71] = (1, 0, rows - 1, 5.0, 13, 0, 12.0, 35.0)
    secs[0, 2, 3] = (1, 0, rows - 1, 5.0, 18, 0, 20.0, 35.0)
    gt, disp = make_images(1, rows, cols, seed=21, n_rects=20)
    _, want = _core_case(secs, gt, disp, 9.0, 1, 1)
    assert (want["stixel_median"][0, 1] != 0).sum() > 10 and want["stixel_median"][0, 0, 0] != 0
    # (column 1 has pixels >= 1, so its full-height rectangle would have a median had the walk gone on)
    assert want["stixel_median"][0, 1, 71] == 0 and want["stixel_median"][0, 2, 3] == 0
    assert len(want["packed"][0]) == 1 + rows + 2


def test_more_keys_than_capacity_fail_the_call():
    rows, cols, C, S = 37, 40, 5, 9
    secs = make_sections(2, C, S, rows, 8, seed=31, inst_class=13, p_inst=0.7, centres=2)
    gt, disp = make_images(2, rows, cols, seed=31)
    gt[1, 0, :9] = [24000 + i for i in range(9)]              # frame 1: at least nine keys
    want = idr.run(secs, gt, disp, 14.0, 2, 3)
    keys = int(want["key_count"][1])
    assert keys >= 9 and want["key_count"][0] < keys
    call = CoreCall(secs, gt, disp, capacity=keys - 1).run(14.0, 2, 3)
    assert call.key_count[:2].cpu().numpy().tolist() == want["key_count"].tolist()   # the TRUE counts
    assert call.untouched()                                    # no frame's labels, flags or triples changed
    call = CoreCall(secs, gt, disp, capacity=keys).run(14.0, 2, 3)
    call.check(want)


def test_a_class_beyond_the_lds_path():
    """64 x 4096, constructed Sections: more than 2048 candidates of one class are clustered out of global memory."""
    rows, cols, C, S = 64, 4096, 512, 12
    secs = make_sections(1, C, S, rows, 8, seed=41, inst_class=13, p_inst=0.9, centres=40)
    gt, disp = make_images(1, rows, cols, seed=41, n_rects=60, numbers=3)
    call, want = _core_case(secs, gt, disp, 5.0, 3, 1)
    idx, lab, _ = want["per_class"][0][2]
    assert len(idx) > 2048 and (lab >= 0).sum() > 100 and (lab == -1).sum() > 100 and lab.max() >= 3


# ---- the edges the clustering shares with k_cluster_instances (is_dbscan.h) ----------------------------------------
def test_the_lds_boundary_with_candidates_that_take_no_part():
    """64 x 2048, 256 columns of 9 slots.  Frame 0 holds exactly 2048 candidates of class 13, the last size clustered
    out of the LDS copies; frame 1 exactly 2049 of class 15, the first size clustered out of global memory (a frame
    has 2304 slots, so the two sizes are two frames).  In both, candidates over stuff have the median 0 and take no
    part, next to clustered ones and to noise."""
    frames = [banded_frame(256, [(13, 2048)], 32, seed=1), banded_frame(256, [(15, 2049)], 32, seed=2)]
    secs, gt, disp = (np.stack(x) for x in zip(*frames))
    assert gt.shape == (2, 64, 2048)
    _, want = _core_case(secs, gt, disp, **BANDED)
    for f, cls, n in ((0, 13, 2048), (1, 15, 2049)):
        lab, part = class_labels(want, f, cls)
        assert len(lab) == n and sum(len(v[0]) for v in want["per_class"][f]) == n
        assert (lab >= 0).sum() > 0 and ((lab == -1) & part).sum() > 0 and (~part).sum() > 50


def test_the_rank_scan_at_its_thread_boundaries():
    """Classes of 1, 255, 256 and 257 candidates in one frame: per = ceil(n / 256) changes from 1 to 2 between the last
    two, and at 257 the ranges of the threads from 129 on start beyond n.  Several clusters in each of the three."""
    sizes = [(11, 1), (12, 255), (13, 256), (14, 257)]
    secs, gt, disp = banded_frame(128, sizes, 4, seed=3)
    _, want = _core_case(secs[None], gt[None], disp[None], **BANDED)
    for cls, n in sizes:
        lab, _ = class_labels(want, 0, cls)
        assert len(lab) == n and (n == 1 or lab.max() >= 3)


@pytest.mark.parametrize("n, C", [(300, 64), (2049, 256)])
def test_one_z_for_every_candidate_equals_the_two_coordinate_kernel(n, C):
    """One instance key over the whole image, one non-zero disparity: every candidate has the same z, dz * dz adds
    exactly +0, and labels, flags and packed triples of is_cluster_instance_disparity are, bit for bit, those of
    is_recluster (k_recore + k_cluster_instances) on the same candidates, eps, min_pts and size_filter.  The
    restatement is held to the same equality in test_instance_disparity_cpu.py."""
    torch, dev = _torch()
    secs, gt, disp = banded_frame(C, [(13, n)], 32, seed=n, one_key=True)
    call, want = _core_case(secs[None], gt[None], disp[None], capacity=1, **BANDED)
    lab, part = class_labels(want, 0, 13)
    assert len(lab) == n and part.all() and (lab >= 0).any() and (lab == -1).any()
    params, lut, odr = oracle.host_initialize(make_config("drn_d_22_unary", 64, C * 8, 32))
    params.max_sections = secs.shape[1]
    assert params.cols == C
    ctx = core_mod.Core(params, lut, odr, max_batch=1)
    try:
        cand = call.cand[0].clone()                       # the flags the three-coordinate call wrote
        labels = torch.full_like(call.labels[0], POISON_LABEL)
        packed = torch.full_like(call.packed[0], POISON_PACKED)
        ib = core_mod.InstanceBuffers(call.com[0].data_ptr(), call.idx[0].data_ptr(), cand.data_ptr(),
                                      call.d_per[0].data_ptr(), labels.data_ptr(), packed.data_ptr())
        rc = ctx.recluster_ptr(call.d_sections.data_ptr(), 1, BANDED["eps"], BANDED["min_pts"], BANDED["size_filter"],
                               [ib], stream=torch.cuda.current_stream(dev).cuda_stream)
        assert rc == 0, core_mod.lib().is_last_error().decode()
        torch.cuda.synchronize(dev)
    finally:
        ctx.close()
    assert torch.equal(labels, call.labels[0]) and torch.equal(cand, call.cand[0])
    assert torch.equal(packed, call.packed[0])


# ---- the host class -----------------------------------------------------------------------------------------------
ROWS, COLS, MAX_DIS = 128, 256, 32
CLUSTER = dict(eps=40.0, min_pts=1, size_filter=3)


def _road(case, n):
    return [(f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground) for f in case["frames"][:n]]


def _host_case(preset):
    if ("host", preset) not in _CACHE:
        case = helpers.build_case(preset, ROWS, COLS, MAX_DIS, seed=3, n_images=2)
        disp = np.clip(np.rint(np.nan_to_num(case["disparity"]) * 4), 0, 255).astype(np.uint8)
        disp[np.random.default_rng(2).random(disp.shape) < 0.04] = 0
        _CACHE["host", preset] = case, disp
    return _CACHE["host", preset]


def _sections(data):
    return np.stack([d.sections for d in data])


def _gt_for(sections, maps, seed):
    """A Cityscapes-like ground truth whose instances are runs of five stixel columns of every candidate (at this
    frame size the presets' own clustering labels nothing to synthesize one from)."""
    pseudo = [{k: (k[0] // 5) % 4 for k in m} for m in maps]
    inst = rr.render(sections, ROWS, COLS, pseudo)[2]
    return ir.synth_gt(inst, seed=seed)


def _instance_image(st, n):
    torch, dev = _torch()
    d_inst = torch.zeros((n, ROWS, COLS), dtype=torch.int32, device=dev)
    st.RenderBatch(n, instance=d_inst.data_ptr())
    return d_inst.cpu().numpy()


def _consumers_equal(st, sections, want, gt, d_gt):
    """RenderBatch's instance image and InstanceOverlapBatch's tables equal those fed with the restatement's labels."""
    n = len(sections)
    inst = rr.render(sections, ROWS, COLS, want["mappings"])[2]
    np.testing.assert_array_equal(_instance_image(st, n), inst)
    for got, frame, g in zip(st.InstanceOverlapBatch(n, d_gt.data_ptr()), inst, gt):
        assert got.tobytes() == ir.joint_histogram(frame, g).tobytes()


@pytest.mark.parametrize("preset", ["drn_d_22_unary", "drn_d_38_pairwise"])
def test_host_class_against_the_restatement(preset):
    case, disp = _host_case(preset)
    cfg = case["cfg"]
    st = host.Stixels()
    st.SetConfig(cfg)
    st.Initialize(max_batch=2)
    big, seg = _dev(case["disparity"]), _dev(case["segmentation"])
    data, maps = st.ComputeBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), _road(case, 2))
    sections = _sections(data)
    gt = _gt_for(sections, maps, seed=17)
    want = idr.run(sections, gt, disp, **CLUSTER)
    maps = st.ReclusterBatch(**CLUSTER)           # the 2-D labels of the same three parameters
    assert (want["label_map"] >= 0).any() and any(want["mappings"][i] != maps[i] for i in range(2))
    # host arrays in, mapping and medians out
    got, med = st.ClusterInstanceDisparityBatch(2, gt, disp, **CLUSTER, with_stixel_median=True)
    assert got == want["mappings"]
    np.testing.assert_array_equal(med.view(np.uint32), want["stixel_median"].view(np.uint32))
    assert st.GetInstanceStixels() == want["mappings"][0]
    d_gt, d_disp = _dev(gt), _dev(disp)
    _consumers_equal(st, sections, want, gt, d_gt)
    # resident device arrays, another eps on the same batch: equal to the restatement again, nothing left behind
    other = idr.run(sections, gt, disp, CLUSTER["eps"] * 0.4, CLUSTER["min_pts"], CLUSTER["size_filter"])
    assert other["mappings"] != want["mappings"]
    got, med = st.ClusterInstanceDisparityBatch(2, d_gt.data_ptr(), d_disp.data_ptr(), CLUSTER["eps"] * 0.4,
                                                CLUSTER["min_pts"], CLUSTER["size_filter"])
    assert got == other["mappings"] and med is None
    _consumers_equal(st, sections, other, gt, d_gt)
    # the first frame alone; ReclusterBatch brings the 2-D labels back
    one, _ = st.ClusterInstanceDisparityBatch(1, d_gt.data_ptr(), d_disp.data_ptr(), **CLUSTER)
    assert one == want["mappings"][:1]
    assert st.ReclusterBatch(**CLUSTER) == maps
    # a frame with more ground-truth instances than slots: the call fails, every label stays
    before = _instance_image(st, 2)
    assert not np.array_equal(before, rr.render(sections, ROWS, COLS, want["mappings"])[2])
    st.SetInstanceDisparityCapacity(int(want["key_count"].max()) - 1)
    with pytest.raises(RuntimeError, match=f"holds {int(want['key_count'].max())} ground-truth instances"):
        st.ClusterInstanceDisparityBatch(2, d_gt.data_ptr(), d_disp.data_ptr(), **CLUSTER)
    np.testing.assert_array_equal(_instance_image(st, 2), before)
    st.SetInstanceDisparityCapacity(int(want["key_count"].max()))
    assert st.ClusterInstanceDisparityBatch(2, d_gt.data_ptr(), d_disp.data_ptr(), **CLUSTER)[0] == want["mappings"]
    # refusals
    with pytest.raises(ValueError, match="n_images"):
        st.ClusterInstanceDisparityBatch(3, d_gt.data_ptr(), d_disp.data_ptr(), **CLUSTER)
    with pytest.raises(ValueError, match="null"):
        st.ClusterInstanceDisparityBatch(2, 0, d_disp.data_ptr(), **CLUSTER)
    with pytest.raises(ValueError, match="min_pts"):
        st.ClusterInstanceDisparityBatch(2, d_gt.data_ptr(), d_disp.data_ptr(), 5.0, 0, 3)
    st.ComputeBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), _road(case, 2), with_instances=False)
    with pytest.raises(ValueError, match="needs a compute call with instances"):
        st.ClusterInstanceDisparityBatch(2, d_gt.data_ptr(), d_disp.data_ptr(), **CLUSTER)
    st.close()


def test_the_selected_set_of_a_sweep():
    from instance_stixels_amd import evaluation
    preset = "drn_d_22_unary"
    case, disp = _host_case(preset)
    cfg = case["cfg"]
    sets = [tuple(getattr(c, f) for f in ("prior_weight", "disparity_weight", "segmentation_weight", "instance_weight",
                                         "eps", "min_pts", "size_filter"))
            for c in (cfg, make_config(preset, ROWS, COLS, MAX_DIS, disparity_weight=cfg.disparity_weight * 30))]
    st = host.Stixels()
    st.SetConfig(cfg)
    st.Initialize(max_batch=2)
    big, seg = _dev(case["disparity"]), _dev(case["segmentation"])
    st.SweepBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), _road(case, 2), sets)
    data0, maps0 = st.SweepSections(0)
    data1, maps1 = st.SweepSections(1)
    s0, s1 = _sections(data0), _sections(data1)
    assert not np.array_equal(s0.view(np.uint8), s1.view(np.uint8))
    gt = _gt_for(s1, maps1, seed=23)
    d_gt, d_disp = _dev(gt), _dev(disp)
    want = idr.run(s1, gt, disp, **CLUSTER)
    assert (want["label_map"] >= 0).any()
    st.SelectSweepSet(1)
    got, med = st.ClusterInstanceDisparityBatch(2, d_gt.data_ptr(), d_disp.data_ptr(), **CLUSTER, with_stixel_median=True)
    assert got == want["mappings"]
    np.testing.assert_array_equal(med.view(np.uint32), want["stixel_median"].view(np.uint32))
    _consumers_equal(st, s1, want, gt, d_gt)
    assert st.SweepSections(0)[1] == maps0, "the labels of set 0 changed"
    # instance_disparity_scores: cluster + overlap + AP in one call, equal to the evaluator fed with numpy's tables
    st.ReclusterBatch(cfg.eps, cfg.min_pts, cfg.size_filter)
    scores = evaluation.instance_disparity_scores(st, d_gt.data_ptr(), d_disp.data_ptr(), **CLUSTER)
    inst = rr.render(s1, ROWS, COLS, want["mappings"])[2]
    ev = evaluation.CityscapesInstanceEval()
    ev.add([ir.joint_histogram(i, g) for i, g in zip(inst, gt)])
    ref = ev.result()
    np.testing.assert_array_equal(scores["result"]["ap"], ref["ap"])
    assert scores["result"]["AP"] == ref["AP"] or (np.isnan(scores["result"]["AP"]) and np.isnan(ref["AP"]))
    st.close()
