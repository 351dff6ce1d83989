"""GPU tests of the unary DP along the back-trace's path (k_unary_path, is_k_unary_path.hip; IS_UNARY_PATH).

The walk computes only the table rows k_backtrace visits.  Every case runs the same batch through the tile path
(IS_UNARY_PATH=0, every row) and through the walk with tables requested (IS_UNARY_PATH=2) into tables pre-filled
with a NaN pattern: at every visited row the three costs and indices carry the tile path's bits, every other row
keeps the pattern, and Sections and instance outputs are identical.  IS_UNARY_PATH=3 makes the walk distrust
itself; its repair launches must give the tile path's bits.  The last tests check the automatic routing."""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

FILL_COST = np.uint32(0x7FC0BEEF)  # a quiet NaN no kernel writes
FILL_INDEX = np.int32(-777)


def _core(case, monkeypatch, env):
    from instance_stixels_amd.core import Core
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return Core(case["params"], case["lut"], case["odr"], max_batch=len(case["frames"]))
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _run(core, case, want_tables, prefill=False):
    """core.run with the tables allocated here (pre-filled with the pattern when asked)."""
    import torch
    from instance_stixels_amd.core import InstanceBuffers, SECTION_DTYPE, INSTANCE_CLASSES
    p, cfg = core.params, case["cfg"]
    C, H, S = p.cols, p.rows, p.max_sections
    dev = torch.device("cuda", core.device)
    seg = torch.from_numpy(np.ascontiguousarray(case["segmentation"], np.int32)).to(dev)
    n = seg.shape[0]
    stream = torch.cuda.current_stream(dev).cuda_stream
    big = torch.from_numpy(np.ascontiguousarray(case["disparity"], np.float32)).to(dev)
    joined = torch.empty((n, C, H), dtype=torch.float32, device=dev)
    core.join_columns_ptr(big.data_ptr(), big.shape[2], bool(cfg.median_join), joined.data_ptr(), n, stream)
    sections = torch.empty((n, C, S, 8), dtype=torch.int32, device=dev)
    cost = index = None
    if want_tables:
        cost = torch.full((n, C, H, 3), int(FILL_COST.view(np.int32)), dtype=torch.int32, device=dev)
        index = torch.full((n, C, H, 3), int(FILL_INDEX), dtype=torch.int32, device=dev)
    com = torch.zeros((n, INSTANCE_CLASSES, C * S, 2), dtype=torch.float32, device=dev)
    idx = torch.zeros((n, INSTANCE_CLASSES, C * S, 2), dtype=torch.int32, device=dev)
    cor = torch.zeros((n, INSTANCE_CLASSES, C * S), dtype=torch.uint8, device=dev)
    per = torch.zeros((n, INSTANCE_CLASSES), dtype=torch.int32, device=dev)
    lab = torch.full((n, INSTANCE_CLASSES, C * S), -9, dtype=torch.int32, device=dev)
    inst = [InstanceBuffers(com[i].data_ptr(), idx[i].data_ptr(), cor[i].data_ptr(), per[i].data_ptr(),
                            lab[i].data_ptr(), None) for i in range(n)]
    core.compute_ptr(joined.data_ptr(), seg.data_ptr(), case["gf"], case["ng"], case["ig"], case["vhor"], False, n,
                     sections.data_ptr(), inst, cost.data_ptr() if cost is not None else None,
                     index.data_ptr() if index is not None else None, stream)
    torch.cuda.synchronize(dev)
    out = dict(sections=sections.cpu().numpy().view(SECTION_DTYPE).reshape(n, C, S),
               inst=[t.cpu().numpy() for t in (com, idx, cor, per, lab)], joined=joined.cpu().numpy())
    if want_tables:
        out["cost_bits"] = cost.cpu().numpy().view(np.uint32)
        out["index_table"] = index.cpu().numpy()
    return out


def _visited(sec_col, H):
    """The rows k_backtrace reads in a unary column: H - 1, and vB - 1 of every Section with vB > 0."""
    n = helpers.n_sections(sec_col)
    rows = {H - 1}
    rows.update(int(v) - 1 for v in sec_col["vB"][:n] if v > 0)
    return sorted(rows)


def _same_outputs(a, b):
    for img in range(len(a["sections"])):
        assert helpers.sections_equal(a["sections"][img], b["sections"][img]), f"image {img}: Sections differ"
    for x, y in zip(a["inst"], b["inst"]):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


def _check_case(case, monkeypatch, extra_env=None, oracle_cols=()):
    env = dict(extra_env or {})
    tile_core = _core(case, monkeypatch, dict(env, IS_UNARY_PATH="0"))
    try:
        tile = _run(tile_core, case, want_tables=True)
        assert tile_core.unary_path()[0] == 0
    finally:
        tile_core.close()
    path_core = _core(case, monkeypatch, dict(env, IS_UNARY_PATH="2"))
    try:
        path = _run(path_core, case, want_tables=True, prefill=True)
        assert path_core.unary_path() == (1, 0)
    finally:
        path_core.close()
    _same_outputs(tile, path)
    H = int(case["cfg"].rows)
    n, C = path["index_table"].shape[:2]
    for img in range(n):
        for c in range(C):
            rows = _visited(tile["sections"][img][c], H)
            mask = np.zeros(H, bool)
            mask[rows] = True
            pc, tc = path["cost_bits"][img, c], tile["cost_bits"][img, c]
            pi, ti = path["index_table"][img, c], tile["index_table"][img, c]
            assert np.array_equal(pc[mask], tc[mask]), f"image {img} column {c}: visited costs differ"
            assert np.array_equal(pi[mask], ti[mask]), f"image {img} column {c}: visited indices differ"
            if not (pi[~mask] == FILL_INDEX).any():  # a generic-encoding column: k_dp_unary fills every row
                assert np.array_equal(pc, tc) and np.array_equal(pi, ti), f"image {img} column {c}: generic column"
                continue
            assert (pc[~mask] == FILL_COST).all() and (pi[~mask] == FILL_INDEX).all(), \
                f"image {img} column {c}: a row the back-trace does not visit was written"
    for img, c in oracle_cols:
        ref = helpers.run_oracle(case, image=img, col_range=(c, c + 1), joined=path["joined"][img])
        errs = helpers.compare(ref, path, img, case["cfg"], cols=[c], check_tables=False)
        assert not errs, "\n".join(errs[:5])
    return tile


CASES = [
    ("drn_d_22_unary", 1024, 2048, 128, {}, 8),              # the headline shape
    ("drn_d_22_unary", 256, 512, 64, {}, 2),
    ("drn_d_22_unary", 256, 512, 256, {}, 2),
    ("drn_d_22_unary", 136, 128, 48, dict(median_join=True), 3),  # H % 32 != 0, D not 2^k
    ("drn_d_22_unary", 200, 256, 128, dict(invalid_disparity=0.0), 2),
    ("drn_d_22_unary", 784, 1792, 128, dict(invalid_disparity=0.0), 2),
    ("disparity_only_unary", 512, 1024, 64, {}, 2),
]


@pytest.mark.parametrize("preset,H,W,D,ov,frames", CASES)
def test_visited_rows_carry_the_tile_path_bits(preset, H, W, D, ov, frames, monkeypatch):
    case = helpers.build_case(preset, H, W, D, seed=71, n_images=frames, **ov)
    _check_case(case, monkeypatch, oracle_cols=((0, 0), (0, case["cfg"].realcols // 2), (frames - 1, 5)))


@pytest.mark.parametrize("family", ["scene", "iid_noise", "low_confidence", "flat_disparity", "homogeneous",
                                    "many_thin_objects", "noisy_disparity", "cityscapes_like"])
def test_visited_rows_on_every_input_family(family, monkeypatch):
    from instance_stixels_amd import synthetic
    from oracle import oracle
    base = helpers.build_case("drn_d_22_unary", 512, 1024, 128, seed=5, n_images=1)
    cfg = base["cfg"]
    frames = [synthetic.make_frame(cfg, seed=400 + i, family=family) for i in range(2)]
    ground = [oracle.host_ground(cfg, f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground) for f in frames]
    case = dict(base, frames=frames, gf=np.stack([g[0] for g in ground]), ng=np.stack([g[1] for g in ground]),
                ig=np.stack([g[2] for g in ground]), vhor=np.array([g[3] for g in ground], np.int32),
                disparity=np.stack([f.disparity for f in frames]),
                segmentation=np.stack([f.segmentation for f in frames]))
    _check_case(case, monkeypatch, oracle_cols=((1, 3),))


def test_visited_rows_with_pruning_off(monkeypatch):
    case = helpers.build_case("drn_d_22_unary", 256, 512, 128, seed=13, n_images=2)
    _check_case(case, monkeypatch, extra_env={"IS_NO_PRUNE": "1"})


@pytest.mark.parametrize("seed", [3, 4])
def test_visited_rows_on_hostile_and_random_inputs(seed, monkeypatch):
    rng = np.random.default_rng(seed)
    H = int(rng.choice([96, 168, 256]))
    D = int(rng.choice([32, 64, 100]))
    ov = dict(invalid_disparity=0.0) if seed % 2 else {}
    case = helpers.build_case("drn_d_22_unary", H, 256, D, seed=seed, n_images=2,
                              disparity_weight=float(rng.uniform(0.002, 0.02)),
                              segmentation_weight=float(rng.uniform(5, 20)), **ov)
    helpers.make_hostile(case, seed)  # generic-encoding columns among FAST ones
    _check_case(case, monkeypatch, oracle_cols=((0, 1), (1, 7)))


def test_forced_distrust_repairs_to_the_same_bits(monkeypatch):
    case = helpers.build_case("drn_d_22_unary", 256, 512, 128, seed=17, n_images=2)
    tile_core = _core(case, monkeypatch, dict(IS_UNARY_PATH="0"))
    try:
        tile = _run(tile_core, case, want_tables=True)
    finally:
        tile_core.close()
    core = _core(case, monkeypatch, dict(IS_UNARY_PATH="3"))
    try:
        for call in (1, 2):
            rep = _run(core, case, want_tables=True, prefill=True)
            assert core.unary_path() == (1, call)
            assert np.array_equal(rep["cost_bits"], tile["cost_bits"])  # the repair writes every row
            assert np.array_equal(rep["index_table"], tile["index_table"])
            _same_outputs(tile, rep)
    finally:
        core.close()


def test_automatic_routing(monkeypatch):
    monkeypatch.delenv("IS_UNARY_PATH", raising=False)
    monkeypatch.delenv("IS_LUT_FUSED", raising=False)
    case = helpers.build_case("drn_d_22_unary", 1024, 2048, 128, seed=23, n_images=2)
    case = helpers.sub_case(case, [i % 2 for i in range(8)])  # 2048 columns
    core = _core(case, monkeypatch, {})
    try:
        assert core.unary_path()[0] == -1
        no_tables = _run(core, case, want_tables=False)
        assert core.unary_path() == (1, 0), "the headline size without tables takes the walk"
        tables = _run(core, case, want_tables=True)
        assert core.unary_path()[0] == 0, "tables requested: the tile path"
        _same_outputs(no_tables, tables)
        core.set_eval_counters(True)
        _run(core, case, want_tables=False)
        assert core.unary_path()[0] == 0, "evaluation counters on: the tile path"
        core.set_eval_counters(False)
        one = helpers.sub_case(case, [0])
        _run(core, one, want_tables=False)
        assert core.unary_path()[0] == 0, "one frame per call: below the threshold"
    finally:
        core.close()
    fused = _core(case, monkeypatch, dict(IS_LUT_FUSED="2"))
    try:
        _run(fused, case, want_tables=False)
        assert fused.unary_path()[0] == 0, "IS_LUT_FUSED=2 tests the fused launch: the tile path"
    finally:
        fused.close()
