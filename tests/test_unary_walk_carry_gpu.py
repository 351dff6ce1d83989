"""GPU tests of the walk's object table (k_unary_path): its prepare launch stores only the LUT's block carries and the
walk rebuilds the entries it reads; the launches behind it that read the complete table (k_dp_unary for the generic
columns, the repair) build it first for the columns they take.  Every case against the tile path's bits or the
oracle."""
import numpy as np
import pytest

import helpers
from test_unary_path_gpu import _core, _run, _same_outputs, _check_case

pytestmark = pytest.mark.gpu


def _headline(seed, hostile):
    case = helpers.build_case("drn_d_22_unary", 1024, 2048, 128, seed=seed, n_images=2)
    if hostile:  # generic-encoding columns among FAST ones
        helpers.make_hostile(case, seed)
    return helpers.sub_case(case, [i % 2 for i in range(8)])  # 2048 columns: the walk by default


def _tile(case, monkeypatch, want_tables):
    core = _core(case, monkeypatch, dict(IS_UNARY_PATH="0"))
    try:
        return _run(core, case, want_tables=want_tables)
    finally:
        core.close()


def test_default_walk_with_generic_columns(monkeypatch):
    monkeypatch.delenv("IS_UNARY_PATH", raising=False)
    monkeypatch.delenv("IS_LUT_FUSED", raising=False)
    case = _headline(31, hostile=True)
    core = _core(case, monkeypatch, {})
    try:
        walk = _run(core, case, want_tables=False)
        assert core.unary_path() == (1, 0)
    finally:
        core.close()
    _same_outputs(_tile(case, monkeypatch, want_tables=False), walk)
    cfg = case["cfg"]
    for img, c in ((0, 0), (1, 1), (1, cfg.realcols // 2), (0, cfg.realcols - 1)):
        ref = helpers.run_oracle(case, image=img, col_range=(c, c + 1), joined=walk["joined"][img])
        errs = helpers.compare(ref, walk, img, cfg, cols=[c], check_tables=False)
        assert not errs, "\n".join(errs[:5])


def test_forced_repair_at_the_headline_size(monkeypatch):
    case = _headline(37, hostile=True)
    tile = _tile(case, monkeypatch, want_tables=True)
    core = _core(case, monkeypatch, dict(IS_UNARY_PATH="3"))
    try:
        rep = _run(core, case, want_tables=True, prefill=True)
        assert core.unary_path() == (1, 1)
    finally:
        core.close()
    assert np.array_equal(rep["cost_bits"], tile["cost_bits"])
    assert np.array_equal(rep["index_table"], tile["index_table"])
    _same_outputs(tile, rep)


def test_tile_call_after_a_walk_call_has_complete_tables(monkeypatch):
    from oracle import oracle
    monkeypatch.delenv("IS_UNARY_PATH", raising=False)
    monkeypatch.delenv("IS_LUT_FUSED", raising=False)
    case = _headline(41, hostile=False)
    tile = _tile(case, monkeypatch, want_tables=True)
    core = _core(case, monkeypatch, dict(IS_LUT_FUSED="0"))  # (the object table in the prepare launch: readable)
    try:
        _run(core, case, want_tables=False)
        assert core.unary_path() == (1, 0)
        got = _run(core, case, want_tables=True)
        assert core.unary_path() == (0, 0), "a call with tables takes the tile path"
        p, cfg = case["params"], case["cfg"]
        for img, c in ((0, 3), (1, cfg.realcols - 2)):
            want = oracle.object_lut_column(p, got["joined"][img][c], case["lut"])[:, : cfg.rows + 1]
            lut = core.read_object_lut(img * cfg.realcols + c)
            assert np.array_equal(helpers.bits(want.T), helpers.bits(lut)), (img, c)
    finally:
        core.close()
    assert np.array_equal(got["cost_bits"], tile["cost_bits"])
    assert np.array_equal(got["index_table"], tile["index_table"])
    _same_outputs(tile, got)


@pytest.mark.parametrize("family", ["scene", "iid_noise", "low_confidence", "flat_disparity", "homogeneous",
                                    "many_thin_objects", "noisy_disparity", "cityscapes_like"])
def test_visited_rows_on_every_family_at_the_headline_shape(family, monkeypatch):
    from instance_stixels_amd import synthetic
    from oracle import oracle
    base = helpers.build_case("drn_d_22_unary", 1024, 2048, 128, seed=5, n_images=1)
    cfg = base["cfg"]
    frames = [synthetic.make_frame(cfg, seed=900 + i, family=family) for i in range(2)]
    ground = [oracle.host_ground(cfg, f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground) for f in frames]
    case = dict(base, frames=frames, gf=np.stack([g[0] for g in ground]), ng=np.stack([g[1] for g in ground]),
                ig=np.stack([g[2] for g in ground]), vhor=np.array([g[3] for g in ground], np.int32),
                disparity=np.stack([f.disparity for f in frames]),
                segmentation=np.stack([f.segmentation for f in frames]))
    _check_case(case, monkeypatch, oracle_cols=((1, 7),))
