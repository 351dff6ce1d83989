"""GPU tests of the Sections k_unary_path writes itself (CallPlan::walk_sections) and of the gated k_backtrace.

A walk call without instance outputs lets the walk emit the Sections of the columns it takes; k_backtrace then runs
gated (generic-encoding columns, every column of a distrusted call).  Once the object type of a row has closed, the
walk's steps load chunks 0 / 4 / 5 of the candidate records and evaluate the ground and sky terms alone
(eval_segment_gs).  Every case runs one batch through the tile path (IS_UNARY_PATH=0) and through the walk
(IS_UNARY_PATH=1; 3 = every call distrusted) into zero-filled Section buffers and compares the two outputs as whole
int32 arrays -- no tolerance -- and columns of the walk's output with the CPU oracle.  There is no host build of the
is_kernels.h helpers, so this comparison is also the pin of eval_segment_gs against eval_segment.

The new steps run in these tests.  Diagnostic build of the walk (a counting buffer behind a -D switch that the
default build does not carry), taken once per input: full steps | steps after the object close | their share.
  families (2 x 512x1024x128): scene 8990 | 2673 | 0.23; iid_noise 18771 | 261 | 0.01; low_confidence 18704 | 728 |
    0.04; flat_disparity 8994 | 2678 | 0.23; homogeneous 2179 | 3167 | 0.59; many_thin_objects 9460 | 2341 | 0.20;
    noisy_disparity 8972 | 2679 | 0.23; cityscapes_like 3660 | 1417 | 0.28
  SHAPES: 200x256x128 inv 960 | 195; 784x1792x128 inv 23750 | 8149; 136x128x48 370 | 0 (none: does not count);
    200x256x64 962 | 203; 256x512 (D = 64 / 128 / 256) 2356 | 433; 1024x2048x128 34662 | 12906 (0.27)
  horizons (6 x 256x512x128, per image vhor = 0 / 255 / 17 / 63 / 192 / 247): scene 144 / 0 / 154 / 144 / 0 / 0 steps
    after the close, homogeneous 64 / 0 / 64 / 64 / 0 / 0, cityscapes_like 23 / 0 / 6 / 0 / 0 / 0: a horizon in the
    lowest block or at H - 1 leaves no such step (the object type stays open in rows that short), the images with
    the horizon in the first block do
  seed 29 (mixed) 3526 | 607; seed 17 (distrust) 2324 | 431; max_sections 2 / 3 / 5: 256 | 90, 384 | 201, 763 | 274;
    seed 41 (two calls) 3516 | 588
  for scale, 16 scene frames of the bench shape: 283447 | 103147 (0.27), 94 steps and 57 rows per column.
"""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu


def _core(case, monkeypatch, env, max_batch=None):
    from instance_stixels_amd.core import Core
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return Core(case["params"], case["lut"], case["odr"], max_batch=max_batch or len(case["frames"]))
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _run(core, case, want_inst=False):
    """One unary call into zero-filled outputs: (Sections as [n][C][S][8] int32, instance arrays or None)."""
    import torch
    from instance_stixels_amd.core import InstanceBuffers, INSTANCE_CLASSES
    p, cfg = core.params, case["cfg"]
    C, H, S = p.cols, p.rows, p.max_sections
    dev = torch.device("cuda", core.device)
    seg = torch.from_numpy(np.ascontiguousarray(case["segmentation"], np.int32)).to(dev)
    n = seg.shape[0]
    stream = torch.cuda.current_stream(dev).cuda_stream
    big = torch.from_numpy(np.ascontiguousarray(case["disparity"], np.float32)).to(dev)
    joined = torch.empty((n, C, H), dtype=torch.float32, device=dev)
    core.join_columns_ptr(big.data_ptr(), big.shape[2], bool(cfg.median_join), joined.data_ptr(), n, stream)
    sections = torch.zeros((n, C, S, 8), dtype=torch.int32, device=dev)
    inst = tensors = None
    if want_inst:
        com = torch.zeros((n, INSTANCE_CLASSES, C * S, 2), dtype=torch.float32, device=dev)
        idx = torch.zeros((n, INSTANCE_CLASSES, C * S, 2), dtype=torch.int32, device=dev)
        cor = torch.zeros((n, INSTANCE_CLASSES, C * S), dtype=torch.uint8, device=dev)
        per = torch.zeros((n, INSTANCE_CLASSES), dtype=torch.int32, device=dev)
        tensors = (com, idx, cor, per)
        inst = [InstanceBuffers(com[i].data_ptr(), idx[i].data_ptr(), cor[i].data_ptr(), per[i].data_ptr(), None,
                                None) for i in range(n)]
    core.compute_ptr(joined.data_ptr(), seg.data_ptr(), case["gf"], case["ng"], case["ig"], case["vhor"], False, n,
                     sections.data_ptr(), inst, None, None, stream)
    torch.cuda.synchronize(dev)
    return (sections.cpu().numpy(), None if tensors is None else [t.cpu().numpy() for t in tensors],
            joined.cpu().numpy())


def _oracle_check(case, sections, joined, cols):
    from instance_stixels_amd.core import SECTION_DTYPE
    n, C, S = sections.shape[:3]
    got = dict(sections=sections.view(SECTION_DTYPE).reshape(n, C, S), joined=joined)
    for img, c in cols:
        ref = helpers.run_oracle(case, image=img, col_range=(c, c + 1), joined=joined[img])
        errs = helpers.compare(ref, got, img, case["cfg"], cols=[c], check_tables=False)
        assert not errs, "\n".join(errs[:5])


def _check(case, monkeypatch, walk="1", oracle_cols=(), extra_env=None, repaired=0):
    env = dict(extra_env or {})
    tile_core = _core(case, monkeypatch, dict(env, IS_UNARY_PATH="0"))
    try:
        tile, _, _ = _run(tile_core, case)
        assert tile_core.unary_path()[0] == 0
    finally:
        tile_core.close()
    walk_core = _core(case, monkeypatch, dict(env, IS_UNARY_PATH=walk))
    try:
        got, _, joined = _run(walk_core, case)
        assert walk_core.unary_path() == (1, repaired)
    finally:
        walk_core.close()
    diff = np.argwhere((got != tile).any(axis=(2, 3)))
    assert diff.size == 0, f"Sections differ from the tile path in (image, column) {diff[:8].tolist()}"
    _oracle_check(case, got, joined, oracle_cols)
    return got


def _family_case(family, H=512, W=1024, D=128, n=2, seed=400):
    from instance_stixels_amd import synthetic
    from oracle import oracle
    base = helpers.build_case("drn_d_22_unary", H, W, D, seed=5, n_images=1)
    cfg = base["cfg"]
    frames = [synthetic.make_frame(cfg, seed=seed + i, family=family) for i in range(n)]
    ground = [oracle.host_ground(cfg, f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground) for f in frames]
    return dict(base, frames=frames, gf=np.stack([g[0] for g in ground]), ng=np.stack([g[1] for g in ground]),
                ig=np.stack([g[2] for g in ground]), vhor=np.array([g[3] for g in ground], np.int32),
                disparity=np.stack([f.disparity for f in frames]),
                segmentation=np.stack([f.segmentation for f in frames]))


FAMILIES = ["scene", "iid_noise", "low_confidence", "flat_disparity", "homogeneous", "many_thin_objects",
            "noisy_disparity", "cityscapes_like"]


def test_every_family_of_the_generator_is_covered():
    from instance_stixels_amd import synthetic
    assert sorted(FAMILIES) == sorted(synthetic.FAMILIES)


@pytest.mark.parametrize("family", FAMILIES)
def test_walk_sections_on_every_input_family(family, monkeypatch):
    _check(_family_case(family), monkeypatch, oracle_cols=((0, 0), (1, 3), (1, 77)))


SHAPES = [
    ("drn_d_22_unary", 200, 256, 128, dict(invalid_disparity=0.0)),
    ("drn_d_22_unary", 784, 1792, 128, dict(invalid_disparity=0.0)),
    ("drn_d_22_unary", 136, 128, 48, dict(median_join=True)),  # H % 32 != 0
    ("drn_d_22_unary", 200, 256, 64, {}),                      # H % 64 != 0, H % 32 != 0
    ("drn_d_22_unary", 256, 512, 64, {}),
    ("drn_d_22_unary", 256, 512, 128, {}),
    ("drn_d_22_unary", 256, 512, 256, {}),
    ("drn_d_22_unary", 1024, 2048, 128, {}),                   # the headline shape
]


@pytest.mark.parametrize("preset,H,W,D,ov", SHAPES)
def test_walk_sections_on_shapes(preset, H, W, D, ov, monkeypatch):
    case = helpers.build_case(preset, H, W, D, seed=71, n_images=2, **ov)
    _check(case, monkeypatch, oracle_cols=((0, 0), (0, case["cfg"].realcols // 2), (1, 5)))


@pytest.mark.parametrize("family", ["scene", "homogeneous", "cityscapes_like"])
def test_walk_sections_with_the_horizon_at_the_edges(family, monkeypatch):
    """Horizon rows 0, H - 1 and inside the first and the last 64-row block: rows where ground never opens
    (every row at or above the horizon) and rows where no sky candidate is left."""
    H = 256
    case = _family_case(family, H=H, W=512, D=128, n=6, seed=900)
    case["vhor"] = np.array([0, H - 1, 17, 63, H - 64, H - 9], np.int32)
    _check(case, monkeypatch, oracle_cols=tuple((i, 11 + i) for i in range(6)))


def test_walk_sections_mixed_fast_and_generic_columns(monkeypatch):
    """One negative class value in some columns: those are generic-encoding columns, which the gated k_backtrace
    writes -- and only those; the others come from the walk."""
    case = helpers.build_case("drn_d_22_unary", 256, 512, 128, seed=29, n_images=3)
    C = case["cfg"].realcols
    generic = [(0, 0), (0, 1), (0, C - 1), (1, 7), (2, C // 2)] + [(2, c) for c in range(20, 40, 3)]
    for img, c in generic:
        case["segmentation"][img, c, 0, 0] = -1
    _check(case, monkeypatch, oracle_cols=((0, 0), (0, 2), (2, C // 2), (2, 21)))


def test_walk_sections_every_call_distrusted(monkeypatch):
    """IS_UNARY_PATH=3: the repair launches and the then ungated k_backtrace overwrite every column."""
    case = helpers.build_case("drn_d_22_unary", 256, 512, 128, seed=17, n_images=2)
    _check(case, monkeypatch, walk="3", repaired=1, oracle_cols=((1, 9),))


@pytest.mark.parametrize("S", [2, 3, 5])
def test_walk_sections_stop_at_max_sections(S, monkeypatch):
    """A small max_sections: the n == S - 1 stop ends most chains before vB = 0."""
    case = helpers.build_case("drn_d_22_unary", 256, 512, 128, seed=31, n_images=2)
    case["params"].max_sections = S
    got = _check(case, monkeypatch)
    from instance_stixels_amd.core import SECTION_DTYPE
    sec = got.view(SECTION_DTYPE).reshape(got.shape[:3])
    cut = sum(1 for img in sec for col in img if helpers.n_sections(col) == S - 1 and col["vB"][S - 2] > 0)
    assert cut > 0, "no chain was cut by max_sections: the case does not reach the stop"


def test_instance_outputs_keep_the_ungated_backtrace(monkeypatch):
    """A walk call with instance outputs: Sections and the candidates per class equal the tile path's."""
    case = helpers.build_case("drn_d_22_unary", 256, 512, 128, seed=37, n_images=2)
    out = {}
    for mode in ("0", "1"):
        core = _core(case, monkeypatch, dict(IS_UNARY_PATH=mode))
        try:
            out[mode] = _run(core, case, want_inst=True)
            assert core.unary_path() == (int(mode), 0)
        finally:
            core.close()
    assert np.array_equal(out["0"][0], out["1"][0])
    for a, b in zip(out["0"][1], out["1"][1]):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    assert int(out["1"][1][3].sum()) > 0, "the case has no instance candidate"


def test_second_call_with_fewer_images(monkeypatch):
    """Two calls on one context, the second with fewer images and without the first call's generic columns: no
    stale Sections, the generic count and the distrust word are clear."""
    case = helpers.build_case("drn_d_22_unary", 256, 512, 128, seed=41, n_images=3)
    for c in (3, 4, 40):
        case["segmentation"][2, c, 0, 0] = -1
    small = helpers.sub_case(case, [1])
    tile_core = _core(small, monkeypatch, dict(IS_UNARY_PATH="0"))
    try:
        tile, _, _ = _run(tile_core, small)
    finally:
        tile_core.close()
    for mode, repaired in (("1", 0), ("3", 2)):
        core = _core(case, monkeypatch, dict(IS_UNARY_PATH=mode), max_batch=3)
        try:
            _run(core, case)
            got, _, joined = _run(core, small)
            assert core.unary_path() == (1, repaired)
            assert np.array_equal(got, tile), f"IS_UNARY_PATH={mode}: the second call differs from the tile path"
            _oracle_check(small, got, joined, ((0, 3), (0, 40)))
        finally:
            core.close()
