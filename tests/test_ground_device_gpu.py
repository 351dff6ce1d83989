"""The device-resident road chain on the MI355X: is_road_choose_batch (k_road_choose), is_compute_road
(k_ground_model + the launches of is_compute), RoadEstimation::ComputeBatchDevice + Stixels::ComputeBatchRoad.

Every device result is compared BITWISE with its host twin -- RoadEstimation::ChooseLineShared,
Stixels::PrecomputeGroundShared -- and the DP with is_compute fed with the twin's arrays.  Six frames of 256 x 512 x
64: five of tests/test_road_batch_gpu.py's recipe, moved up or down by a few rows so that their horizons differ, and
one of zeros (no lines).  SEED was chosen on the CPU (the roads below need no GPU): on it PrecomputeGroundShared and
PrecomputeGround agree bitwise for all six roads, which test_host_chain asserts before it relies on it."""
import ctypes

import numpy as np
import pytest

import frontend_reference
import helpers
from instance_stixels_amd import core, host

pytestmark = pytest.mark.gpu

ROWS, COLS, D, N = 256, 512, 64, 6
SEED = ROWS + D
SHIFT = (0, 9, -6, 14, -11)   # rows each frame is moved down (up): five horizons
THR, HOUGH_THR = 0.2, 25      # RoadEstimation::Initialize


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def _frames():
    """Five frames as test_road_batch_gpu._batch builds them (two presets, hostile columns in every third, zeros
    sprinkled into every fourth + 1), each moved by SHIFT rows; then the frame of zeros."""
    frames, cases = [], []
    for i in range(N - 1):
        preset = ("drn_d_22_unary", "drn_d_38_pairwise")[i % 2]
        case = helpers.build_case(preset, ROWS, COLS, D, seed=SEED + 17 * i)
        if i % 3 == 2:
            case = helpers.make_hostile(case, SEED + i)
        d = case["disparity"][0].copy()
        if i % 4 == 1:
            d[::7, ::5] = 0.0
        k = SHIFT[i]
        if k > 0:
            d = np.concatenate([np.zeros((k, COLS), np.float32), d[:-k]])
        elif k < 0:
            d = np.concatenate([d[-k:], np.repeat(d[-1:], -k, 0)])
        frames.append(d)
        cases.append(case)
    frames.append(np.zeros((ROWS, COLS), np.float32))
    return np.stack(frames), cases


class Scene:
    def __init__(self):
        self.disp, self.cases = _frames()
        self.cfgs = (self.cases[0]["cfg"], self.cases[1]["cfg"])            # unary, pairwise
        cfg = self.cfgs[0]
        self.cam = (cfg.camera_center_y * ROWS / 1024, cfg.baseline, cfg.focal)
        f0 = self.cases[0]["frames"][0]                                     # the calibration: every frame's fallback
        self.fallback = (int(f0.vhor_image), np.float32(f0.camera_tilt), np.float32(f0.camera_height),
                         np.float32(f0.alpha_ground))
        seg = [c["segmentation"][0] for c in self.cases]
        assert all(s.shape == seg[0].shape for s in seg)
        self.seg = np.stack(seg + [np.zeros_like(seg[0])])
        # the roads of the six frames on the CPU: binary v-disparity, host Hough transform, the shared line choice
        self.lines, self.status, self.roads = [], [], []
        for d in self.disp:
            _, binary, _ = frontend_reference.vdisparity(d, D, THR)
            lines = host.hough_lines(binary, cap=1 << 16)
            st, _, road = host.choose_line_shared(lines, len(lines), 0, 512, *self.cam, ROWS, fallback=self.fallback)
            self.lines.append(lines), self.status.append(st), self.roads.append(road)
        assert self.status == [core.ROAD_OK] * 5 + [core.ROAD_NONE]
        assert len({r[0] for r in self.roads[:5]}) == 5, "the five roads have different horizons"
        self.road_records = np.array(self.roads, core.ROAD_DTYPE)
        self.vhor_lib = np.array([ROWS - r[0] - 1 for r in self.roads], np.int32)
        self._ground = {}

    def stixels(self, pairwise):
        st = host.Stixels()
        st.SetConfig(self.cfgs[int(pairwise)])
        return st

    def shared_ground(self, pairwise):
        """PrecomputeGroundShared of the six roads: (function, normalization, inv_sigma2) [6][ROWS] each"""
        if pairwise not in self._ground:
            st = self.stixels(pairwise)
            st.PrecomputeHost()
            g = [st.PrecomputeGroundShared(int(v), *r[1:])[:3] for v, r in zip(self.vhor_lib, self.roads)]
            self._ground[pairwise] = (tuple(np.stack([x[k] for x in g]) for k in range(3)), st.GroundParams(),
                                      st.GetLogLUT())
            st.close()
        return self._ground[pairwise]

    def core(self, pairwise, max_batch=N):
        case = self.cases[int(pairwise)]
        c = core.Core(case["params"], case["lut"], case["odr"], max_batch=max_batch)
        _, gp, lut = self.shared_ground(pairwise)
        c.set_ground_model(gp, lut)
        return c


@pytest.fixture(scope="module")
def scene():
    return Scene()


# ---------------------------------------------------------------- is_road_choose_batch

def _choose(L, ctx, scene, lines, total, over, max_lines, n=N):
    import torch
    dev = lines.device
    road = torch.full((n, 4), -77, dtype=torch.int32, device=dev)
    status = torch.full((n,), 99, dtype=torch.uint8, device=dev)
    lo, hi = host.pitch_gate()
    rc = core.road_choose_batch_ptr(ctx, n, lines.data_ptr(), total.data_ptr(), over.data_ptr(), max_lines,
                                    *scene.cam, lo, hi, scene.fallback, road.data_ptr(), status.data_ptr(), None)
    assert rc == 0, L.is_last_error()
    torch.cuda.synchronize()
    return road.cpu().numpy().view(core.ROAD_DTYPE).reshape(n), status.cpu().numpy()


def _check_against_twin(scene, road, status, lines, total, over, max_lines):
    fb = np.array([scene.fallback], core.ROAD_DTYPE)
    for i in range(len(status)):
        kept = lines[i][:max(min(int(total[i]), max_lines), 0)]
        st, _, want = host.choose_line_shared(kept, int(total[i]), int(over[i]), max_lines, *scene.cam, ROWS,
                                              fallback=scene.fallback)
        assert status[i] == st, (i, status[i], st)
        assert road[i].tobytes() == np.array([want], core.ROAD_DTYPE).tobytes(), (i, road[i], want)
        if st != core.ROAD_OK:
            assert road[i].tobytes() == fb.tobytes(), i


def test_road_choose_batch_equals_choose_line_shared(scene):
    import torch
    dev = torch.device("cuda", 0)
    L = core.lib()
    ctx = ctypes.c_void_p()
    assert L.is_road_ctx_create(ctypes.byref(ctx), ROWS, COLS, D, N, -1) == 0, L.is_last_error()
    d = torch.from_numpy(scene.disp).to(dev)
    assert L.is_road_vdisparity_batch(ctx, d.data_ptr(), N, ctypes.c_float(THR), None, None, None, None) == 0
    seen = {}
    for max_lines in (512, 1):   # everything the transform found; only the best line
        lines = torch.full((N, max_lines, 2), float("nan"), dtype=torch.float32, device=dev)
        total = torch.full((N,), -1, dtype=torch.int32, device=dev)
        over = torch.full((N,), -1, dtype=torch.int32, device=dev)
        assert L.is_road_hough_batch(ctx, N, HOUGH_THR, max_lines, 8192, lines.data_ptr(), None, total.data_ptr(),
                                     over.data_ptr(), None) == 0, L.is_last_error()
        road, status = _choose(L, ctx, scene, lines, total, over, max_lines)
        _check_against_twin(scene, road, status, lines.cpu().numpy(), total.cpu().numpy(), over.cpu().numpy(), max_lines)
        seen[max_lines] = status.tolist()
        if max_lines == 512:   # the CPU's lines are the device's: the scene's roads are this call's
            assert status.tolist() == scene.status
            assert road.tobytes() == scene.road_records.tobytes()
    # frame 1's best line is the sky's (rejected): with one line kept the device cannot decide it
    assert seen[1][1] == core.ROAD_UNDECIDED and seen[512][1] == core.ROAD_OK
    assert seen[1][5] == core.ROAD_NONE

    # hand-written lines: what no synthetic frame produces
    step = np.float32(np.pi / 180)
    th = lambda n: np.float32(0.0) + np.float32(n) * step   # noqa: E731
    cy, _, focal = scene.cam
    good = [100.0, th(80)]
    far = [np.float32((cy + 0.9 * focal) * np.sin(np.float64(th(90)))), th(90)]   # pitch 42 degrees, horizon below the image
    M = 128
    hand = np.full((N, M, 2), np.nan, np.float32)
    total = np.zeros(N, np.int32)
    over = np.zeros(N, np.int32)
    def put(i, rows, tot=None, ov=0):   # noqa: E306
        hand[i, :len(rows)] = rows
        total[i], over[i] = len(rows) if tot is None else tot, ov
    put(0, [[5.0, th(0)], [0.0, th(0)], [-30.0, th(0)], good])                       # rho / 0, 0 / 0 in front
    put(1, [far, good])                                                              # accepted, horizon outside: 3
    put(2, [good], ov=1)                                                             # overflow: no line is looked at
    put(3, [[10.0, np.nan], [10.0, 1.0], [np.inf, th(45)], [10.0, th(0)]])           # nothing acceptable: 0
    put(4, [[7.0, th(0)]] * 100 + [[-100.0, th(80)]])                                # the second round of the wave; |rho|
    put(5, [[7.0, th(0)]] * M, tot=M + 5)                                            # more lines than kept: 2
    t = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    road, status = _choose(L, ctx, scene, t(hand), t(total), t(over), M)
    _check_against_twin(scene, road, status, hand, total, over, M)
    assert status.tolist() == [core.ROAD_OK, core.ROAD_HORIZON, core.ROAD_UNDECIDED, core.ROAD_NONE, core.ROAD_OK,
                               core.ROAD_UNDECIDED]
    assert road[4].tobytes() == road[0].tobytes()
    assert {0, 1, 2, 3} <= set(seen[1]) | set(seen[512]) | set(status.tolist())
    assert L.is_road_ctx_destroy(ctx) == 0


# ---------------------------------------------------------------- is_compute_road: the ground model and the DP

def test_compute_road_builds_the_shared_ground_model(scene):
    (fn, norm, is2), _, _ = scene.shared_ground(False)
    c = scene.core(False)
    try:
        c.run(disparity_big=scene.disp, segmentation=scene.seg, pairwise=False, road=scene.road_records,
              want_instances=False)
        for i in range(N):
            got, vhor = c.read_ground(i)
            assert vhor == scene.vhor_lib[i], i
            for k, want in enumerate((fn[i], norm[i], is2[i])):
                assert np.array_equal(_bits(got[k]), _bits(want)), (i, k, np.argwhere(_bits(got[k]) != _bits(want))[:4])
            assert np.isneginf(got[1][vhor:]).any(), i   # rows at and above the horizon: FastLog(0) = -inf
    finally:
        c.close()


def _same_outputs(a, b, n, tables):
    for i in range(n):
        assert helpers.sections_equal(a["sections"][i], b["sections"][i]), i
        assert np.array_equal(a["inst_per_class"][i], b["inst_per_class"][i]), i
        for cls in range(8):
            m = int(a["inst_per_class"][i][cls])
            for name in ("inst_centerofmass", "inst_indices", "inst_core", "inst_labels"):
                assert np.array_equal(a[name][i][cls][:m].view(np.uint8), b[name][i][cls][:m].view(np.uint8)), (i, name)
    if tables:
        assert np.array_equal(_bits(a["cost_table"]), _bits(b["cost_table"]))
        assert np.array_equal(a["index_table"], b["index_table"])


@pytest.mark.parametrize("pairwise", [False, True])
@pytest.mark.parametrize("n", [1, N])
def test_compute_road_equals_compute_on_the_shared_model(scene, pairwise, n):
    (fn, norm, is2), _, _ = scene.shared_ground(pairwise)
    c = scene.core(pairwise)
    try:
        kw = dict(disparity_big=scene.disp[:n], segmentation=scene.seg[:n], pairwise=pairwise, want_tables=True)
        want = c.run(ground_function=fn[:n], normalization_ground=norm[:n], inv_sigma2_ground=is2[:n],
                     vhor=scene.vhor_lib[:n], **kw)
        for hint in (-1, int(scene.vhor_lib[:n].min())):
            got = c.run(road=scene.road_records[:n], vhor_min_hint=hint, **kw)
            _same_outputs(got, want, n, tables=True)
        assert sum(helpers.n_sections(col) for col in want["sections"][0]) > COLS // 8   # (not an empty result)
    finally:
        c.close()


def test_compute_road_on_the_unary_walk(scene, monkeypatch):
    """A unary call without tables at any size (IS_UNARY_PATH=1): the launch path of large batches."""
    monkeypatch.setenv("IS_UNARY_PATH", "1")
    (fn, norm, is2), _, _ = scene.shared_ground(False)
    c = scene.core(False)
    try:
        kw = dict(disparity_big=scene.disp, segmentation=scene.seg, pairwise=False, want_tables=False)
        want = c.run(ground_function=fn, normalization_ground=norm, inv_sigma2_ground=is2, vhor=scene.vhor_lib, **kw)
        assert c.unary_path()[0] == 1
        got = c.run(road=scene.road_records, **kw)
        assert c.unary_path()[0] == 1
        _same_outputs(got, want, N, tables=False)
    finally:
        c.close()


def test_compute_road_plans_the_pairwise_windows_from_the_hint(scene):
    """4096 columns per call: from there pairwise phase 1 stages fn windows in the tiles below the smallest horizon
    -- the one launch decision that reads the horizons.  Unknown (-1: no windowed tile), the true minimum, and
    is_compute's own plan give the same bits."""
    reps = 64
    idx = np.arange(reps) % N
    (fn, norm, is2), _, _ = scene.shared_ground(True)
    c = scene.core(True, max_batch=reps)
    try:
        assert reps * c.params.cols >= 4096
        kw = dict(disparity_big=scene.disp[idx], segmentation=scene.seg[idx], pairwise=True, want_tables=False)
        want = c.run(ground_function=fn[idx], normalization_ground=norm[idx], inv_sigma2_ground=is2[idx],
                     vhor=scene.vhor_lib[idx], **kw)
        for hint in (-1, int(scene.vhor_lib.min())):
            _same_outputs(c.run(road=scene.road_records[idx], vhor_min_hint=hint, **kw), want, reps, tables=False)
    finally:
        c.close()


@pytest.mark.parametrize("preset", ["drn_d_22_unary", "drn_d_38_pairwise"])
def test_compute_road_on_the_smallest_golden_shape(preset):
    case = helpers.build_case(preset, 64, 64, 32, seed=3)
    cfg, f = case["cfg"], case["frames"][0]
    st = host.Stixels()
    st.SetConfig(cfg)
    st.PrecomputeHost()
    vhor_lib = 64 - f.vhor_image - 1
    fn, norm, is2, _ = st.PrecomputeGroundShared(vhor_lib, f.camera_tilt, f.camera_height, f.alpha_ground)
    road = np.array([(f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground)], core.ROAD_DTYPE)
    c = core.Core(case["params"], case["lut"], case["odr"], max_batch=1)
    try:
        c.set_ground_model(st.GroundParams(), st.GetLogLUT())
        kw = dict(disparity_big=case["disparity"], segmentation=case["segmentation"], pairwise=bool(cfg.pairwise),
                  want_tables=True)
        want = c.run(ground_function=fn[None], normalization_ground=norm[None], inv_sigma2_ground=is2[None],
                     vhor=np.array([vhor_lib], np.int32), **kw)
        _same_outputs(c.run(road=road, **kw), want, 1, tables=True)
    finally:
        c.close()
        st.close()


def test_compute_road_needs_the_ground_model(scene):
    case = scene.cases[0]
    c = core.Core(case["params"], case["lut"], case["odr"], max_batch=1)
    try:
        with pytest.raises(core.CoreError, match="is_ctx_set_ground_model"):
            c.run(disparity_big=scene.disp[:1], segmentation=scene.seg[:1], pairwise=False,
                  road=scene.road_records[:1])
    finally:
        c.close()


# ---------------------------------------------------------------- the host classes

def _world_and_render(st, n):
    import torch
    dev = torch.device("cuda", 0)
    offsets, records = st.WorldBatch(n)
    label = torch.zeros((n, ROWS, COLS), dtype=torch.uint8, device=dev)
    disp = torch.zeros((n, ROWS, COLS), dtype=torch.float32, device=dev)
    inst = torch.zeros((n, ROWS, COLS), dtype=torch.int32, device=dev)
    st.RenderBatch(n, label=label.data_ptr(), disparity=disp.data_ptr(), instance=inst.data_ptr())
    torch.cuda.synchronize()
    return offsets.copy(), records.copy().tobytes(), label.cpu().numpy(), _bits(disp.cpu().numpy()), inst.cpu().numpy()


def _same_batch(a, b, n):
    (data_a, maps_a, extra_a), (data_b, maps_b, extra_b) = a, b
    for i in range(n):
        assert helpers.sections_equal(data_a[i].sections, data_b[i].sections), i
        ha, hb = vars(data_a[i]).copy(), vars(data_b[i]).copy()
        ha.pop("sections"), hb.pop("sections")
        assert _bits(ha.pop("alpha_ground")) == _bits(hb.pop("alpha_ground")) and ha == hb, (i, ha, hb)
        assert maps_a[i] == maps_b[i], i
    for x, y in zip(extra_a, extra_b):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y


@pytest.mark.parametrize("pairwise", [False, True])
def test_host_chain(scene, pairwise):
    import torch
    dev = torch.device("cuda", 0)
    d_big = torch.from_numpy(scene.disp).to(dev)
    d_seg = torch.from_numpy(np.ascontiguousarray(scene.seg, np.int32)).to(dev)
    d_road = torch.full((N, 4), -77, dtype=torch.int32, device=dev)
    d_status = torch.full((N,), 99, dtype=torch.uint8, device=dev)
    re_ = host.RoadEstimation()
    re_.Initialize(*scene.cam, ROWS, COLS, D)
    st = scene.stixels(pairwise)
    st.Initialize(max_batch=N)
    try:
        chain = torch.cuda.Stream(dev)   # one queue for both objects: nothing between the launches but the order
        torch.cuda.synchronize()

        def new_chain(n):
            d_road.fill_(-77), d_status.fill_(99)
            torch.cuda.synchronize()
            re_.ComputeBatchDevice(d_big.data_ptr(), n, d_road.data_ptr(), d_status.data_ptr(), scene.fallback,
                                   stream=chain.cuda_stream)
            data, maps, road, status = st.ComputeBatchRoad(pairwise, n, d_big.data_ptr(), d_seg.data_ptr(),
                                                           d_road.data_ptr(), d_status.data_ptr(),
                                                           stream=chain.cuda_stream)
            return (data, maps, _world_and_render(st, n)), road, status

        def legacy(road):
            data, maps = st.ComputeBatch(pairwise, d_big.data_ptr(), d_seg.data_ptr(), road)
            return data, maps, _world_and_render(st, len(road))

        new, road, status = new_chain(N)
        assert status == scene.status
        assert np.array(road, core.ROAD_DTYPE).tobytes() == scene.road_records.tobytes()
        for i in range(N):   # what the chain returned is what its headers and consumers use
            assert new[0][i].vhor == ROWS - road[i][0] - 1 and _bits(new[0][i].alpha_ground) == _bits(road[i][3])
        # the precondition of the comparison below, checked on the host: on these roads the two ground models agree
        for i in range(N):
            st.SetRoadParameters(int(road[i][0]), *(float(x) for x in road[i][1:]))
            legacy_model = st.GetGroundModel()
            shared_model = st.PrecomputeGroundShared(legacy_model[3], *road[i][1:])
            assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(legacy_model[:3], shared_model[:3])), i
        want = legacy(road)
        _same_batch(new, want, N)
        # a second call with fewer frames, and the legacy call afterwards on the same object
        new3, road3, status3 = new_chain(3)
        assert road3 == road[:3] and status3 == status[:3]
        _same_batch(new3, (want[0][:3], want[1][:3], _world_and_render_of(want, st, pairwise, d_big, d_seg, road[:3])), 3)
        again = legacy(road)
        _same_batch(again, want, N)

        # measured, not asserted: the new chain against the legacy chain (libm's atanf / cosf / erff) on the frames
        # the legacy chain can compute -- it reports the frame of zeros as not ok with a road of zeros, which callers
        # skip: a camera height of 0 is outside the domain of the host's PrecomputeGround
        road_l, ok_l = re_.ComputeBatch(d_big.data_ptr(), N)
        assert ok_l == [True] * (N - 1) + [False]
        data_l, _ = st.ComputeBatch(pairwise, d_big.data_ptr(), d_seg.data_ptr(), road_l[:N - 1])
        differ = total = 0
        for i in range(N - 1):
            for c in range(st.GetRealCols()):
                a, b = new[0][i].sections[c], data_l[i].sections[c]
                na, nb = helpers.n_sections(a), helpers.n_sections(b)
                total += max(na, nb)
                m = min(na, nb)
                differ += abs(na - nb) + int((a[:m].view(np.int32).reshape(m, 8) != b[:m].view(np.int32).reshape(m, 8))
                                             .any(axis=1).sum())
        same_roads = sum(np.array([a], core.ROAD_DTYPE).tobytes() == np.array([b], core.ROAD_DTYPE).tobytes()
                         for a, b in zip(road_l[:N - 1], road[:N - 1]))
        print(f"{'pairwise' if pairwise else 'unary'}: {differ} of {total} Sections of the {N - 1} frames with a road "
              f"differ between the device-resident chain and the legacy chain ({same_roads} of {N - 1} roads are "
              f"bitwise equal); the sixth frame has no road: status {status[N - 1]}, the fallback in place")
    finally:
        st.close()
        re_.close()


def _world_and_render_of(want, st, pairwise, d_big, d_seg, road):
    """the consumers' outputs of a legacy call over the first frames only"""
    st.ComputeBatch(pairwise, d_big.data_ptr(), d_seg.data_ptr(), road)
    return _world_and_render(st, len(road))
