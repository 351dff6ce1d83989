"""The HIP path and the CPU oracle against the upstream reference's OWN code, hipified and built for
gfx950 into oracle/_ref/libref_stixels.so (`make -C oracle ref`, oracle/ref_driver.hip, numerics
substitutions in oracle/ref_shim.h).  Every case compares three results -- reference, oracle, HIP --
bit for bit: Sections (vT, vB, type, class, cost / disparity / instance-centre bits), the joined
disparity, the object LUT rows 0..H, and the instance candidates per class as a multiset (the
reference appends them in atomic arrival order, StixelsKernels.cu:927-944).

This closes the common-mode gap of the rest of the suite: the oracle and the kernels were written by
one author from one reading of the reference, so they could agree with each other and both differ
from it."""
import ctypes

import numpy as np
import pytest

import helpers
from instance_stixels_amd import synthetic
from oracle import oracle, reference

pytestmark = pytest.mark.gpu

if not reference.available():
    pytest.skip(f"{reference.LIB_PATH} is not built (`make -C oracle ref` needs a checkout of the upstream "
                "reference)", allow_module_level=True)

PRESETS = ["drn_d_22_unary", "drn_d_38_unary", "drn_d_22_pairwise", "drn_d_38_pairwise",
           "disparity_only_unary", "disparity_only_pairwise"]


def _as_got(out):
    return dict(joined=out["joined"][None], sections=out["sections"][None])


def _assert_candidates(ref, other, image=None, what="oracle"):
    want = other["inst_per_class"] if image is None else other["inst_per_class"][image]
    assert np.array_equal(ref["inst_per_class"], want), (ref["inst_per_class"].tolist(), want.tolist(), what)
    for cls in range(reference.INSTANCE_CLASSES):
        a, b = reference.candidate_multiset(ref, cls), reference.candidate_multiset(other, cls, image)
        assert np.array_equal(a, b), f"instance candidates of class {cls}: reference vs {what}"


def _three_way(case, image=0, hip=None, ref=None):
    """Reference vs oracle vs HIP on one frame of a case; returns the reference's result."""
    cfg = case["cfg"]
    if ref is None:
        ref = reference.stixels_compute_frame(case, image)
    assert ref["vhor"] == int(case["vhor"][image])
    orc = helpers.run_oracle(case, image=image)
    errs = helpers.compare(orc, _as_got(ref), 0, cfg, check_tables=False)
    assert not errs, "reference vs oracle:\n" + "\n".join(errs[:10])
    _assert_candidates(ref, orc)
    if hip is not None:
        errs = helpers.compare(orc, hip, image, cfg, check_tables=False)
        assert not errs, "HIP vs oracle:\n" + "\n".join(errs[:10])
        assert helpers.sections_equal(ref["sections"], hip["sections"][image])
        _assert_candidates(ref, hip, image, "HIP")
    return ref


def _run_hip(case, **kw):
    return helpers.run_core(case, want_tables=False, **kw)


@pytest.mark.parametrize("median", [False, True])
@pytest.mark.parametrize("inv", [-1.0, 0.0])
@pytest.mark.parametrize("preset", PRESETS)
def test_presets_small_frame(preset, inv, median):
    case = helpers.build_case(preset, 64, 64, 32, seed=11, invalid_disparity=inv, median_join=median)
    _three_way(case, hip=_run_hip(case))


@pytest.mark.parametrize("preset,shape", [
    (p, s) for s in [(136, 128, 48), (256, 512, 256), (512, 1024, 64), (784, 1792, 128), (1024, 2048, 128)]
    for p in ("drn_d_22_unary", "drn_d_38_pairwise")] + [("drn_d_38_pairwise", (1024, 1024, 256))])
def test_frame_shapes(preset, shape):
    """H % 32 != 0 and D not a power of two (136 x 128 x 48), D = rows (256), the reference's own
    operating point with invalid_disparity = 0 (784 x 1792), rows_power2 = 2048 (1024 rows) and
    D = 256 at the largest rows the reference can launch."""
    rows, cols, D = shape
    ov = dict(invalid_disparity=0.0) if rows == 784 else {}
    case = helpers.build_case(preset, rows, cols, D, seed=rows + D, **ov)
    _three_way(case, hip=_run_hip(case))


@pytest.mark.parametrize("D", [2, 3, 5, 7, 33, 34, 63, 65, 66, 127, 129, 130, 136])
@pytest.mark.parametrize("preset", ["drn_d_22_unary", "drn_d_38_pairwise"])
def test_disparity_counts_where_the_dp_changes_path(preset, D):
    """The oracle that tests/test_disparity_axis_gpu.py trusts, pinned on the reference at the counts of its table that
    lie in the reference's domain (1 <= max_dis <= rows): fewer than four disparities, counts that are no multiple of 4
    on either side of 32, 64 and 128, and D = rows at a row count that is no power of two.  136 x 64, the ramp columns
    of that test (bins 0 and D - 1 are reached by a mean; all values inside [0, D))."""
    case = helpers.ramp_columns(helpers.build_case(preset, 136, 64, D, seed=D))
    assert helpers.reaches_both_end_bins(oracle.join_columns(case["cfg"], case["disparity"][0]), D)
    _three_way(case, hip=_run_hip(case))


@pytest.mark.parametrize("family", synthetic.FAMILIES)
def test_input_families(family):
    preset = ("drn_d_22_unary", "drn_d_38_pairwise")[synthetic.FAMILIES.index(family) % 2]
    case = helpers.build_case(preset, 512, 1024, 128, seed=5)
    cfg = case["cfg"]
    f = synthetic.make_frame(cfg, seed=600, family=family)
    g = oracle.host_ground(cfg, f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground)
    case["frames"] = [f]
    case["gf"][0], case["ng"][0], case["ig"][0], case["vhor"][0] = g
    case["disparity"][0], case["segmentation"][0] = f.disparity, f.segmentation
    _three_way(case, hip=_run_hip(case))


@pytest.mark.parametrize("k", range(6))
def test_hostile_inputs(k):
    """Negative class values, offsets whose squares wrap int32, class totals near 2^24, tiny and
    subnormal disparities: StixelsKernel only sums and compares these (never indexes with them)."""
    preset = ("drn_d_22_unary", "drn_d_38_pairwise", "drn_d_38_unary")[k % 3]
    ov = dict(invalid_disparity=0.0) if k >= 3 else {}
    case = helpers.make_hostile(helpers.build_case(preset, 128, 256, 32, seed=70 + k, **ov), seed=k)
    _three_way(case, hip=_run_hip(case))


@pytest.mark.parametrize("preset", ["drn_d_22_unary", "drn_d_38_pairwise"])
def test_degenerate_inputs(preset):
    """Columns where candidates tie or the generic encodings take over (test_parity_gpu's degenerate
    frame): all invalid, constant, at the top of the domain, zero / all-equal / huge class values,
    offsets past 2^18, tiny and subnormal disparities."""
    case = helpers.build_case(preset, 128, 128, 32, seed=33, invalid_disparity=0.0)
    d, s = case["disparity"][0], case["segmentation"][0]
    d[:, 0:8], d[:, 8:16], d[:, 16:24], d[64:, 24:32] = 0.0, 5.0, 30.98, 0.0
    s[4] = 0
    s[5, 19:21, :16], s[6, 19:21, :16] = 8 * 4000, -8 * 4000
    s[7, :19, :16] = 0
    s[8, 19:21, :16], s[9, 19:21, :16], s[10, 19, 3] = 8 * 50000, -8 * 50000, 2 ** 30
    s[13, 3, :16], s[14, 12, 5], s[15, :19, :16] = 200000, -7, 130000
    d[:, 88:96], d[40:50, 96:104], d[10, 96:104] = 1e-30, 1e-30, 3.0e-39
    _three_way(case, hip=_run_hip(case))


@pytest.mark.parametrize("vhor_image", [-5, 0, 1, 63, 126, 127, 140])
@pytest.mark.parametrize("preset", ["drn_d_22_unary", "drn_d_38_pairwise"])
def test_horizon_edge_cases(preset, vhor_image):
    case = helpers.build_case(preset, 128, 64, 32, seed=31)
    f = case["frames"][0]
    g = oracle.host_ground(case["cfg"], vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground)
    case["gf"][0], case["ng"][0], case["ig"][0], case["vhor"][0] = g
    ref = reference.stixels_compute(case["cfg"], case["disparity"][0], case["segmentation"][0], vhor_image,
                                    f.camera_tilt, f.camera_height, f.alpha_ground)
    _three_way(case, hip=_run_hip(case), ref=ref)


def _walk_case(seed):
    case = helpers.build_case("drn_d_22_unary", 1024, 2048, 128, seed=seed, n_images=2)
    return helpers.sub_case(case, [i % 2 for i in range(8)])   # 2048 columns: the walk by default


def test_unary_walk_at_its_default_routing(monkeypatch):
    """k_unary_path with the carry-row rebuild of the object table: 8 frames of 1024 x 2048 in one call."""
    from instance_stixels_amd.core import Core
    for var in ("IS_UNARY_PATH", "IS_LUT_FUSED"):
        monkeypatch.delenv(var, raising=False)
    case = _walk_case(17)
    core = Core(case["params"], case["lut"], case["odr"], max_batch=8)
    try:
        hip = core.run(disparity_big=case["disparity"], segmentation=case["segmentation"],
                       ground_function=case["gf"], normalization_ground=case["ng"], inv_sigma2_ground=case["ig"],
                       vhor=case["vhor"], pairwise=False, median_join=False, want_tables=False)
        assert core.unary_path() == (1, 0)
    finally:
        core.close()
    refs = [_three_way(case, image=i, hip=hip) for i in range(2)]
    for i in range(2, 8):
        assert helpers.sections_equal(refs[i % 2]["sections"], hip["sections"][i]), i


def test_unary_tile_path(monkeypatch):
    monkeypatch.setenv("IS_UNARY_PATH", "0")
    case = helpers.sub_case(_walk_case(19), [0, 1])
    hip = _run_hip(case)
    for i in range(2):
        _three_way(case, image=i, hip=hip)


@pytest.mark.parametrize("split", [1, 0])
def test_pairwise_phase2_kernels(split, monkeypatch):
    """IS_P2_SPLIT=1: k_pw_phase2s (chain + evaluator wave); 0: k_pw_phase2 (one wave)."""
    monkeypatch.setenv("IS_P2_SPLIT", str(split))
    case = helpers.build_case("drn_d_38_pairwise", 256, 1536, 64, seed=77 + split, n_images=2)
    hip = _run_hip(case)
    for i in range(2):
        _three_way(case, image=i, hip=hip)


def test_host_class_one_frame():
    from instance_stixels_amd import host
    case = helpers.build_case("drn_d_38_pairwise", 784, 1792, 128, seed=3, invalid_disparity=0.0)
    cfg, f = case["cfg"], case["frames"][0]
    st = host.Stixels()
    st.SetConfig(cfg)
    st.Initialize()
    st.SetDisparityImage(f.disparity)
    st.SetSegmentation(f.segmentation)
    st.SetRoadParameters(f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground)
    data = st.Compute(cfg.pairwise)
    st.Finish()
    ref = _three_way(case)
    assert helpers.sections_equal(ref["sections"], data.sections)


@pytest.mark.parametrize("preset,rows,cols,D,ov", [
    ("drn_d_22_unary", 128, 64, 32, {}), ("drn_d_38_pairwise", 136, 64, 16, dict(invalid_disparity=0.0)),
    ("drn_d_22_unary", 256, 96, 128, {}), ("disparity_only_pairwise", 512, 64, 64, {})])
def test_object_lut(preset, rows, cols, D, ov):
    """d_object_lut after Compute (layout [col][fn][rows_power2 + 1]) against oracle.object_lut_column
    and the HIP prepare kernel's table (Core.read_object_lut), rows 0..H.  Entries above H are never
    read and ComputeObjectLUT leaves those past its n_power2 unwritten: not compared."""
    from instance_stixels_amd.core import Core
    case = helpers.build_case(preset, rows, cols, D, seed=5, **ov)
    cfg, p = case["cfg"], case["params"]
    ref = reference.stixels_compute_frame(case, want_lut=True)
    core = Core(p, case["lut"], case["odr"], max_batch=1)
    try:
        core.run(disparity_big=case["disparity"], segmentation=case["segmentation"], ground_function=case["gf"],
                 normalization_ground=case["ng"], inv_sigma2_ground=case["ig"], vhor=case["vhor"],
                 pairwise=bool(cfg.pairwise), median_join=bool(cfg.median_join), want_tables=False)
        for c in range(cfg.realcols):
            want = helpers.bits(ref["object_lut"][c][:, : rows + 1])                   # [D][H + 1]
            orc = oracle.object_lut_column(p, ref["joined"][c], case["lut"])[:, : rows + 1]
            assert np.array_equal(want, helpers.bits(orc)), c
            assert np.array_equal(want, helpers.bits(core.read_object_lut(c).T)), c
    finally:
        core.close()


@pytest.mark.parametrize("median", [False, True])
@pytest.mark.parametrize("inv", [-1.0, 0.0])
def test_column_join(inv, median):
    """JoinColumns (mean / median, with and without an explicit invalid value) against is_join_columns
    and oracle.join_columns; the frame goes on through the DP as well."""
    case = helpers.build_case("drn_d_38_pairwise", 256, 512, 64, seed=23, invalid_disparity=inv,
                              median_join=median)
    if inv >= 0:
        case["disparity"][0][:, :8] = 0.0          # one all-invalid column
        case["disparity"][0][100:, 8:16] = 0.0     # one half-invalid column
    hip = _run_hip(case)
    ref = reference.stixels_compute_frame(case)
    want = helpers.bits(ref["joined"])
    assert np.array_equal(want, helpers.bits(oracle.join_columns(case["cfg"], case["disparity"][0])))
    assert np.array_equal(want, helpers.bits(hip["joined"][0]))
    _three_way(case, hip=hip, ref=ref)


def test_vdisparity_kernels():
    """ComputeHistogram / ComputeMaximum / ComputeBinaryImage (RoadEstimationKernels.cu) against
    is_road_vdisparity, is_road_vdisparity_batch and oracle.road_vdisparity, on the frames of
    test_road_batch_gpu._batch that lie in the reference's domain (0 <= d < max_dis)."""
    import torch
    from instance_stixels_amd import core
    from test_road_batch_gpu import THR, _batch
    rows, cols, D, n = 256, 512, 64, 8
    disp, _ = _batch(rows, cols, D, n, seed=rows + D)
    keep = [i for i in range(n) if bool(((disp[i] >= 0) & (disp[i] < D)).all())]
    assert len(keep) >= 6
    for i in range(n):
        if i not in keep:
            with pytest.raises(reference.ReferenceError):
                reference.road_vdisparity(disp[i], D, THR)
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(disp).to(dev)
    vd = torch.full((n, rows, D), -1, dtype=torch.int32, device=dev)
    mx = torch.full((n,), -1, dtype=torch.int32, device=dev)
    bn = torch.full((n, rows, D), 7, dtype=torch.uint8, device=dev)
    L = core.lib()
    ctx = ctypes.c_void_p()
    assert L.is_road_ctx_create(ctypes.byref(ctx), rows, cols, D, n, -1) == 0, L.is_last_error()
    try:
        assert L.is_road_vdisparity_batch(ctx, d.data_ptr(), n, ctypes.c_float(THR), vd.data_ptr(),
                                          mx.data_ptr(), bn.data_ptr(), None) == 0, L.is_last_error()
        torch.cuda.synchronize()
    finally:
        L.is_road_ctx_destroy(ctx)
    vd, mx, bn = vd.cpu().numpy(), mx.cpu().numpy(), bn.cpu().numpy()
    for i in keep:
        r_v, r_b, r_m = reference.road_vdisparity(disp[i], D, THR)
        o_v, o_b, o_m = oracle.road_vdisparity(disp[i], D, THR)
        s_v = torch.empty((rows, D), dtype=torch.int32, device=dev)
        s_m = torch.zeros(1, dtype=torch.int32, device=dev)
        s_b = torch.empty((rows, D), dtype=torch.uint8, device=dev)
        assert L.is_road_vdisparity(d[i].data_ptr(), rows, cols, D, ctypes.c_float(THR), s_v.data_ptr(),
                                    s_m.data_ptr(), s_b.data_ptr(), None) == 0
        torch.cuda.synchronize()
        for v, b, m, what in ((o_v, o_b, o_m, "oracle"), (vd[i], bn[i], int(mx[i]), "batch"),
                              (s_v.cpu().numpy(), s_b.cpu().numpy(), int(s_m.item()), "single")):
            assert np.array_equal(r_v, v) and np.array_equal(r_b, b) and r_m == m, (i, what)


def _road_three_way(ours, ref, frame, D, what):
    """One frame through our RoadEstimation::Compute and the reference's, the reference's cv::HoughLines answering
    with OUR host transform of our binary image: the same return value, horizon point and pitch / height / slope
    bits; the call the reference made: the image equal to our binary v-disparity, rho 1, our theta, threshold 25.
    Returns (ok, horizon point, pitch, height, slope) or None where the driver refuses the frame."""
    from hough_reference import THETA
    from instance_stixels_amd import host
    from test_road_batch_gpu import HOUGH_THR, _bits, _oracle_safe
    ok = ours.Compute(frame)
    binary = ours.GetBinaryVDisparity()
    lines = host.hough_lines(binary, cap=1 << 20)
    reference.set_hough_lines(lines)
    if not _oracle_safe(frame, D):     # the reference does not bounds-check its bins: the driver must refuse
        with pytest.raises(reference.ReferenceError) as e:
            ref.Compute(frame)
        assert e.value.code == reference.REF_E_DOMAIN
        return None
    before = reference.hough_call()["calls"]
    assert ref.Compute(frame) == ok, what
    call = reference.hough_call()
    assert call["calls"] == before + 1
    assert call["image"].shape == binary.shape and np.array_equal(call["image"], binary), what
    assert call["type"] == 0 and call["rho"] == 1.0 and call["threshold"] == HOUGH_THR
    assert np.float32(call["theta"]).view(np.int32) == THETA.view(np.int32)      # RoadEstimation.cpp's kPi / 180
    got = (ours.horizon_point, ours.pitch, ours.camera_height, ours.slope)
    if ok:
        assert ours.horizon_point == ref.horizon_point, what
        assert np.array_equal(_bits(got[1:]), _bits([ref.pitch, ref.camera_height, ref.slope])), what
    return (ok,) + got


@pytest.mark.parametrize("shape", [(256, 512, 64), (1024, 2048, 128)])
def test_road_estimation_class(shape):
    """RoadEstimation::Compute and ComputeBatch against the reference's RoadEstimation class (RoadEstimation.cu
    built as it stands; its cv::HoughLines is the stub of oracle/ref_stubs/opencv2 and returns the lines of our
    host transform), on the frames of test_road_batch_gpu._batch that lie in the reference's domain."""
    import torch
    from instance_stixels_amd import host
    from test_road_batch_gpu import _batch, _init, _same
    rows, cols, D = shape
    n = 8
    disp, cases = _batch(rows, cols, D, n, seed=rows + D)
    cfg = cases[0]["cfg"]
    ours, ref = host.RoadEstimation(), reference.RoadEstimation()
    try:
        _init(ours, cfg, rows, cols, D)
        ref.Initialize(cfg.camera_center_y * rows / 1024, cfg.baseline, cfg.focal, rows, cols, D)
        single = [_road_three_way(ours, ref, disp[i], D, i) for i in range(n)]
        keep = [i for i in range(n) if single[i] is not None]
        assert len(keep) >= 6 and any(single[i][0] for i in keep) and not all(single[i][0] for i in keep)
        d = torch.from_numpy(disp[keep]).to(torch.device("cuda", 0))
        road, ok = ours.ComputeBatch(d.data_ptr(), len(keep))
        _same(road, ok, [single[i] for i in keep])
    finally:
        ours.close()
        ref.close()


def test_road_estimation_reinitialize():
    """Another shape and another camera between frames, on both sides (the reference's caller finishes the object
    before it initialises it again; the driver does that)."""
    from instance_stixels_amd import host
    from test_road_batch_gpu import _batch
    a = (256, 512, 64, 128.0, 0.209313, 2262.52)
    b = (128, 256, 32, 70.0, 0.35, 300.0)
    frames = {s: _batch(s[0], s[1], s[2], 2, seed=5 + s[0])[0] for s in (a, b)}
    ours, ref = host.RoadEstimation(), reference.RoadEstimation()
    try:
        seen = []
        for k, s in enumerate((a, b, a, b)):
            rows, cols, D, cy, base, focal = s
            ours.Initialize(cy, base, focal, rows, cols, D)
            ref.Initialize(cy, base, focal, rows, cols, D)
            out = _road_three_way(ours, ref, frames[s][k // 2], D, k)
            assert out is not None and out[0]
            seen.append(out)
        assert seen[0] != seen[1] and seen[2] != seen[3]      # the other camera gives another road
    finally:
        ours.close()
        ref.close()


def _edge_lines(camera, rows, D):
    """Integral (rho, n) pairs that put the pitch just inside and just outside the gate: neighbours in rho at one
    angle of which RoadEstimation::ChooseLine accepts one and refuses the other.  Returns {sign of the pitch:
    (accepted line, refused line)}."""
    from hough_reference import THETA
    from instance_stixels_amd import host
    found = {}
    for n in (1, 2, 3, 5, 10, 30, 60, 90, 120, 150, 170, 177, 178, 179):
        theta = np.float32(n) * THETA
        took = [host.choose_line([[rho, theta]], *camera, rows) for rho in range(0, rows + D + 1)]
        for rho in range(rows + D):
            if (took[rho][0] >= 0) != (took[rho + 1][0] >= 0):
                inside, outside = (rho, rho + 1) if took[rho][0] >= 0 else (rho + 1, rho)
                sign = 1 if took[inside][1][1] > 0 else -1
                found.setdefault(sign, ([inside, theta], [outside, theta]))
    return found


def test_road_line_choice_on_injected_lists():
    """ComputeHough's loop and ComputeCameraProperties (RoadEstimation.cu:136-193) against
    RoadEstimation::ChooseLine on hand-made line lists inside the domain cv::HoughLines can produce: rho integral
    (numrho is odd at resolution 1) and theta = n * THETA.  Non-integral rho is left out on purpose: the
    reference takes `abs` of the float rho unqualified, and which overload that names depends on the headers in
    sight -- the integer one truncates; on integral rho both agree, so only there is the reference's result
    defined for our purposes."""
    from hough_reference import THETA
    from instance_stixels_amd import host
    from test_road_batch_gpu import _batch, _bits
    rows, cols, D = 256, 512, 64
    frame = _batch(rows, cols, D, 1, seed=9)[0][0]

    def t(n):
        return np.float32(n) * THETA

    cameras = [(128.0, 0.209313, 2262.52), (200.0, 0.3, 100.0)]    # the second: both edges of the gate in reach
    ref = reference.RoadEstimation()
    try:
        for camera in cameras:
            ref.Initialize(*camera, rows, cols, D)
            edges = _edge_lines(camera, rows, D)
            assert 1 in edges and (camera[2] > 1000 or -1 in edges), edges
            fail = [[37, t(0)], [0, t(0)], edges[1][1]]          # horizon inf, NaN, pitch past +50 degrees
            assert all(host.choose_line([l], *camera, rows)[0] == -1 for l in fail)
            lists = {
                "n = 0, horizon inf": [[37, t(0)]],
                "n = 0, rho 0, horizon NaN": [[0, t(0)]],
                "n = 90": [[100, t(90)]],
                "negative rho": [[-150, t(100)], [150, t(100)]],
                "negative rho at n = 170": [[-20, t(170)]],
                "three refused, then one": fail + [[120, t(80)], [100, t(90)]],
                "none passes": fail,
                "empty": np.zeros((0, 2), np.float32),
            }
            for sign, (inside, outside) in edges.items():
                lists[f"pitch gate {sign:+d}: outside, inside"] = [outside, inside]
                lists[f"pitch gate {sign:+d}: outside alone"] = [outside]
            accepted = 0
            for what, lines in lists.items():
                lines = np.asarray(lines, np.float32).reshape(-1, 2)
                k, road = host.choose_line(lines, *camera, rows)
                reference.set_hough_lines(lines)
                assert ref.Compute(frame) == (k >= 0), what
                if k < 0:
                    continue
                accepted += 1
                want = np.array([abs(lines[k, 0]), lines[k, 1]], np.float32)     # the same accepted index
                assert np.array_equal(_bits(ref.accepted_line), _bits(want)), what
                assert not any(abs(l[0]) == want[0] and l[1] == want[1] for l in lines[:k]), what
                assert road[0] == ref.horizon_point, what
                assert np.array_equal(_bits(road[1:]), _bits([ref.pitch, ref.camera_height, ref.slope])), what
            assert accepted >= 5
            k = host.choose_line(lists["three refused, then one"], *camera, rows)[0]
            assert k == 3
    finally:
        ref.close()


def test_driver_refuses_inputs_outside_the_domain():
    """The host checks of ref_driver.hip refuse before any launch: the reference's device
    asserts are compiled out, so nothing else stands between these inputs and a launch."""
    case = helpers.build_case("drn_d_22_unary", 64, 64, 32, seed=1)
    cfg, f = case["cfg"], case["frames"][0]

    def run(cfg=cfg, disparity=case["disparity"][0]):
        return reference.stixels_compute(cfg, disparity, case["segmentation"][0], f.vhor_image, f.camera_tilt,
                                         f.camera_height, f.alpha_ground)

    for bad in (-1.0, 32.0, np.nan):
        d = case["disparity"][0].copy()
        d[3, 5] = bad
        with pytest.raises(reference.ReferenceError) as e:
            run(disparity=d)
        assert e.value.code == reference.REF_E_DOMAIN
    from instance_stixels_amd import make_config
    for ov in (dict(column_step=4), dict(rows=1032, max_dis=32), dict(rows=32, max_dis=64)):
        kw = dict(rows=64, cols=64, max_dis=32)
        kw.update(ov)
        bad_cfg = make_config("drn_d_22_unary", kw.pop("rows"), kw.pop("cols"), kw.pop("max_dis"), **kw)
        with pytest.raises(reference.ReferenceError) as e:
            reference.shapes(bad_cfg)
        assert e.value.code == reference.REF_E_DOMAIN
