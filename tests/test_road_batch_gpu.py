"""Batched road estimation on the MI355X (is_k_road.hip, is_road_* of the C ABI, RoadEstimation::ComputeBatch):
every result is compared bitwise with the single-frame path -- the oracle's v-disparity, the host Hough
transform and RoadEstimation::Compute -- on synthetic frames and hostile frames in the same batch."""
import ctypes

import numpy as np
import pytest

import frontend_reference
import helpers
from instance_stixels_amd import core, host
from oracle import oracle

pytestmark = pytest.mark.gpu

THR = 0.2       # road_vdisparity_threshold of RoadEstimation::Initialize
HOUGH_THR = 25  # RoadEstimation's accumulator threshold
N_HOSTILE = 4


def _spiky(rng, rows, cols, D, k=8):
    """Each row holds k random disparity bins: a random cloud of binary pixels with thousands of maxima."""
    d = np.empty((rows, cols), np.float32)
    for i in range(rows):
        bins = rng.choice(np.arange(1, D), k, replace=False)
        d[i] = bins[rng.integers(0, k, cols)] + 0.5
    return d


def _hostile_pos(k, n):
    return (3 * k + 1) % n


def _batch(rows, cols, D, n, seed):
    """n frames: synthetic scenes of several seeds and two presets (some with hostile columns, some with zeros
    sprinkled in) and, for n >= 8, the hostile frames at _hostile_pos(0 .. 3): all zero, sky only (bin 0),
    half the pixels in ignored bins (>= max_dis), random spikes (many maxima)."""
    rng = np.random.default_rng(seed)
    cases, frames = [], []
    i = 0
    while len(frames) < n:
        preset = ("drn_d_22_unary", "drn_d_38_pairwise")[i % 2]
        case = helpers.build_case(preset, rows, cols, D, seed=seed + 17 * i)
        if i % 3 == 2:
            case = helpers.make_hostile(case, seed + i)
        d = case["disparity"][0].copy()
        if i % 4 == 1:
            d[::7, ::5] = 0.0
        frames.append(d)
        cases.append(case)
        i += 1
    if n >= 2 * N_HOSTILE:
        hostile = [np.zeros((rows, cols), np.float32),
                   rng.uniform(0.01, 0.99, (rows, cols)).astype(np.float32),
                   np.where(rng.random((rows, cols)) < 0.5, frames[0],
                            D + rng.uniform(0, 50, (rows, cols))).astype(np.float32),
                   _spiky(rng, rows, cols, D)]
        for k, h in enumerate(hostile):
            frames[_hostile_pos(k, n)] = h
    return np.stack(frames), cases


def _vdisparity_np(d, D, thr):
    """numpy twin of is_road_vdisparity for frames with bins outside [0, D) too (the oracle mirrors the
    reference, which does not check them): the restatement of tests/frontend_reference.py, whose bins are
    stated rule by rule (tests/test_vdisparity_edges_gpu.py feeds it NaN, +-inf and values beyond int32)."""
    return frontend_reference.vdisparity(d, D, thr)


def _oracle_safe(d, D):
    return bool(((d == 0) | ((d >= 0) & (d < D))).all())


def _bits(x):
    return np.asarray(x, np.float32).view(np.int32)


def _init(re_, cfg, rows, cols, D):
    re_.Initialize(cfg.camera_center_y * rows / 1024, cfg.baseline, cfg.focal, rows, cols, D)


def _per_frame(disp, cfg, rows, cols, D):
    re_ = host.RoadEstimation()
    _init(re_, cfg, rows, cols, D)
    out = []
    for f in disp:
        ok = re_.Compute(f)
        out.append((ok, re_.horizon_point, re_.pitch, re_.camera_height, re_.slope))
    re_.close()
    return out


def _same(batch_road, batch_ok, single):
    assert len(batch_road) == len(single) == len(batch_ok)
    for i, (ok, hp, pitch, height, slope) in enumerate(single):
        assert batch_ok[i] == ok, i
        if ok:
            vhor, tilt, h, alpha = batch_road[i]
            assert vhor == hp, i
            assert np.array_equal(_bits([tilt, h, alpha]), _bits([pitch, height, slope])), i
        else:
            assert batch_road[i] == (0, 0.0, 0.0, 0.0), i


@pytest.mark.parametrize("shape", [(256, 512, 64), (1024, 2048, 128), (1024, 4096, 256), (2048, 4096, 256)])
def test_batched_vdisparity_and_hough_match_the_single_frame_path(shape):
    import torch
    rows, cols, D = shape
    n = 8
    disp, _ = _batch(rows, cols, D, n, seed=rows + D)
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(disp).to(dev)
    vd = torch.full((n, rows, D), -1, dtype=torch.int32, device=dev)
    mx = torch.full((n,), -1, dtype=torch.int32, device=dev)
    bn = torch.full((n, rows, D), 7, dtype=torch.uint8, device=dev)
    L = core.lib()
    ctx = ctypes.c_void_p()
    assert L.is_road_ctx_create(ctypes.byref(ctx), rows, cols, D, n, -1) == 0, L.is_last_error()
    assert L.is_road_vdisparity_batch(ctx, d.data_ptr(), n, ctypes.c_float(THR), vd.data_ptr(), mx.data_ptr(),
                                      bn.data_ptr(), None) == 0, L.is_last_error()
    torch.cuda.synchronize()
    vd, mx, bn = vd.cpu().numpy(), mx.cpu().numpy(), bn.cpu().numpy()
    binaries = []
    for i in range(n):
        want_v, want_b, want_m = _vdisparity_np(disp[i], D, THR)
        if _oracle_safe(disp[i], D):
            o_v, o_b, o_m = oracle.road_vdisparity(disp[i], D, THR)
            assert np.array_equal(o_v, want_v) and np.array_equal(o_b, want_b) and o_m == want_m, i
        assert np.array_equal(vd[i], want_v), i
        assert int(mx[i]) == want_m, i
        assert np.array_equal(bn[i], want_b), i
        binaries.append(want_b)
    assert mx[_hostile_pos(0, n)] == 0 and not bn[_hostile_pos(0, n)].any()
    want_lines = [host.hough_lines(b, cap=1 << 20) for b in binaries]

    for max_lines, cap in ((512, 8192), (3, 64)):
        lines = torch.full((n, max_lines, 2), float("nan"), dtype=torch.float32, device=dev)
        votes = torch.zeros((n, max_lines), dtype=torch.int32, device=dev)
        total = torch.full((n,), -1, dtype=torch.int32, device=dev)
        over = torch.full((n,), -1, dtype=torch.int32, device=dev)
        assert L.is_road_hough_batch(ctx, n, HOUGH_THR, max_lines, cap, lines.data_ptr(), votes.data_ptr(),
                                     total.data_ptr(), over.data_ptr(), None) == 0, L.is_last_error()
        torch.cuda.synchronize()
        lines, votes, total, over = (t.cpu().numpy() for t in (lines, votes, total, over))
        for i in range(n):
            want = want_lines[i]
            assert total[i] == len(want), (i, total[i], len(want))
            assert over[i] == int(len(want) > cap), i
            if not over[i]:
                k = min(max_lines, len(want))
                assert np.array_equal(_bits(lines[i, :k]), _bits(want[:k])), i
                assert (np.diff(votes[i, :k]) <= 0).all() and (votes[i, :k] > HOUGH_THR).all(), i
        assert total[_hostile_pos(0, n)] == 0
        if cap == 64:
            assert over[_hostile_pos(3, n)] == 1                       # the spiky frame
        else:
            assert not over[[i for i in range(n) if i != _hostile_pos(3, n)]].any()
    assert L.is_road_ctx_destroy(ctx) == 0


@pytest.mark.parametrize("shape", [(256, 512, 64), (1024, 2048, 128), (1024, 4096, 256)])
def test_compute_batch_equals_compute_per_frame(shape):
    import torch
    rows, cols, D = shape
    sizes = (64, 1, 8) if shape == (1024, 2048, 128) else (8, 1, 12)
    n = max(sizes)
    disp, cases = _batch(rows, cols, D, n, seed=3 * rows + D)
    cfg = cases[0]["cfg"]
    single = _per_frame(disp, cfg, rows, cols, D)
    assert any(s[0] for s in single) and not all(s[0] for s in single)
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(disp).to(dev)
    re_ = host.RoadEstimation()
    _init(re_, cfg, rows, cols, D)
    spiky = _hostile_pos(3, n)
    for m in sizes:                        # repeated calls on one object, n changing (grows, then shrinks)
        road, ok = re_.ComputeBatch(d.data_ptr(), m)
        _same(road, ok, single[:m])
        # the default limits never send a synthetic frame to the host; the spiky frame may go there
        assert re_.GetBatchFallbacks() <= int(spiky < m)
    road, ok = re_.ComputeBatch(d[5].data_ptr(), 1)       # a later frame alone
    _same(road, ok, single[5:6])
    # one line and a small candidate buffer: the host Hough transform decides what the device cannot
    re_.SetBatchLimits(1, 16)
    road, ok = re_.ComputeBatch(d.data_ptr(), 8)
    _same(road, ok, single[:8])
    assert re_.GetBatchFallbacks() > 0
    re_.close()


def test_batched_road_parameters_drive_stixels_compute_batch():
    import torch
    rows, cols, D, n = 256, 512, 64, 4
    case = helpers.build_case("drn_d_22_unary", rows, cols, D, seed=71, n_images=n)
    cfg = case["cfg"]
    single = _per_frame(case["disparity"], cfg, rows, cols, D)
    assert all(s[0] for s in single)
    dev = torch.device("cuda", 0)
    big = torch.from_numpy(case["disparity"]).to(dev)
    seg = torch.from_numpy(case["segmentation"]).to(dev)
    re_ = host.RoadEstimation()
    _init(re_, cfg, rows, cols, D)
    road, ok = re_.ComputeBatch(big.data_ptr(), n)
    re_.close()
    assert all(ok)
    per_frame = [(hp, pitch, height, slope) for _, hp, pitch, height, slope in single]
    st = host.Stixels()
    st.SetConfig(cfg)
    st.Initialize(max_batch=n)
    got, got_maps = st.ComputeBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), road)
    want, want_maps = st.ComputeBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), per_frame)
    st.close()
    for i in range(n):
        assert got[i].sections.tobytes() == want[i].sections.tobytes(), i
        assert got[i].vhor == want[i].vhor and got_maps[i] == want_maps[i], i


def test_compute_batch_on_a_set_device_restores_the_current_device():
    import torch
    rows, cols, D, n = 256, 512, 64, 4
    case = helpers.build_case("drn_d_22_unary", rows, cols, D, seed=9, n_images=n)
    cfg = case["cfg"]
    single = _per_frame(case["disparity"], cfg, rows, cols, D)
    other = torch.cuda.device_count() - 1          # 0 on a one-GPU machine
    d = torch.from_numpy(case["disparity"]).to(torch.device("cuda", 0))
    torch.cuda.set_device(other)
    try:
        re_ = host.RoadEstimation()
        re_.SetDevice(0)
        _init(re_, cfg, rows, cols, D)
        assert re_.GetActiveDevice() == 0
        road, ok = re_.ComputeBatch(d.data_ptr(), n)
        assert torch.cuda.current_device() == other
        _same(road, ok, single)
        re_.close()
        assert torch.cuda.current_device() == other
    finally:
        torch.cuda.set_device(0)


# Frames of _batch(rows, cols, D, 8, seed=rows + D) whose deciding line stands alone: the first line of the float64
# reference's list that passes the pitch gate is a certain peak and its lo exceeds hi of every other possible peak
# that passes the gate (so every list inside the bounds leads to it).  The others are the all-zero frame (1), the
# sky-only frame (4: one column of pixels, refused by the gate).  STRICT: the frames where that line outvotes every
# other possible peak, gated or not (in the larger shapes the sky column's line comes first and is refused).
DECIDED = (0, 2, 3, 5, 6, 7)
STRICT = {256: (0, 2, 3, 5, 6, 7), 1024: (2,), 2048: ()}


@pytest.mark.parametrize("shape", [(256, 512, 64), (1024, 2048, 128), (2048, 4096, 256)])
def test_device_hough_against_the_float64_reference(shape):
    """k_road_hough / k_road_sort against tests/hough_reference.py, a witness that shares nothing with the host
    transform they are otherwise compared with: lines and votes of 8 frames inside the reference's bounds, and
    the road parameters of the deciding line where the reference says it stands alone."""
    import torch
    from hough_reference import Hough
    rows, cols, D = shape
    n, max_lines, cap = 8, 4096, 8192
    disp, cases = _batch(rows, cols, D, n, seed=rows + D)
    cfg = cases[0]["cfg"]
    camera = (cfg.camera_center_y * rows / 1024, cfg.baseline, cfg.focal)
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(disp).to(dev)
    bn = torch.full((n, rows, D), 7, dtype=torch.uint8, device=dev)
    lines = torch.full((n, max_lines, 2), float("nan"), dtype=torch.float32, device=dev)
    votes = torch.zeros((n, max_lines), dtype=torch.int32, device=dev)
    total = torch.full((n,), -1, dtype=torch.int32, device=dev)
    over = torch.full((n,), -1, dtype=torch.int32, device=dev)
    L = core.lib()
    ctx = ctypes.c_void_p()
    assert L.is_road_ctx_create(ctypes.byref(ctx), rows, cols, D, n, -1) == 0, L.is_last_error()
    try:
        assert L.is_road_vdisparity_batch(ctx, d.data_ptr(), n, ctypes.c_float(THR), None, None, bn.data_ptr(),
                                          None) == 0, L.is_last_error()
        assert L.is_road_hough_batch(ctx, n, HOUGH_THR, max_lines, cap, lines.data_ptr(), votes.data_ptr(),
                                     total.data_ptr(), over.data_ptr(), None) == 0, L.is_last_error()
        torch.cuda.synchronize()
    finally:
        L.is_road_ctx_destroy(ctx)
    bn, lines, votes, total, over = (t.cpu().numpy() for t in (bn, lines, votes, total, over))
    decided, strict = [], []
    for i in range(n):
        assert np.array_equal(bn[i], _vdisparity_np(disp[i], D, THR)[1]), i
        h = Hough(bn[i], threshold=HOUGH_THR)
        certain, possible = int(h.certain_peaks().sum()), int(h.possible_peaks().sum())
        print(f"{shape} frame {i}: points {h.n_points} ambiguous {h.n_ambiguous} certain {certain} "
              f"possible {possible} device {total[i]}")
        assert possible <= min(max_lines, cap) and not over[i], i
        assert certain <= total[i] <= possible, i
        got = lines[i, :total[i]]
        h.check_lines(got, votes[i, :total[i]])
        # the line that decides the road
        want, wn, wr, _ = h.lines()
        k, road = host.choose_line(want, *camera, rows)
        if k < 0:
            assert i not in DECIDED, i
            continue
        pn, pr = np.nonzero(h.possible_peaks())
        gated = np.zeros((h.numangle, h.numrho), bool)
        for a, c, l in zip(pn, pr, h.line(pn, pr)):
            gated[a, c] = host.choose_line(l, *camera, rows)[0] == 0
        if h.dominant(wn[k], wr[k]):
            strict.append(i)
        if h.dominant(wn[k], wr[k], among=gated):
            decided.append(i)
            k_got, road_got = host.choose_line(got, *camera, rows)
            assert k_got >= 0 and np.array_equal(_bits(got[k_got]), _bits(want[k])), i
            assert road_got[0] == road[0] and np.array_equal(_bits(road_got[1:]), _bits(road[1:])), i
            if i in strict:
                assert k_got == 0, i
    assert tuple(decided) == DECIDED and tuple(strict) == STRICT[rows], (decided, strict)
