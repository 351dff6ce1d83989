"""GPU tests of the carry rows a walk call builds from a cost table in LDS (k_lut_carry, CallPlan::lut_carry_lds): at
max_dis <= 128 the prepare step of a walk call is k_prepare_columns + k_lut_carry, at max_dis = 256 it stays
k_prepare_fused<CARRY>.  On both routes the carries lutC[k][fn] must carry the bits of rows 32 k of the oracle's object
table and of the tile path's table (the prepare launch of an IS_UNARY_PATH=0 context), in every column."""
import functools

import numpy as np
import pytest

import helpers
from oracle import oracle
from test_unary_path_gpu import _core, _run

pytestmark = pytest.mark.gpu

# (preset, rows, cols, D, overrides, images, hostile)
SHAPES = {
    "one_block_masked_lanes": ("drn_d_22_unary", 32, 48, 48, {}, 1, False),       # only carry 0; D < 64
    "partial_last_block": ("drn_d_22_unary", 104, 64, 64, {}, 1, False),          # H % 32 != 0; NF = 1, full wave
    "two_fn_odd_columns": ("drn_d_22_unary", 96, 40, 128, {}, 3, False),          # NF = 2; 15 columns
    "invalid_value": ("drn_d_22_unary", 136, 64, 64, dict(invalid_disparity=0.0), 1, False),
    "hostile": ("drn_d_22_unary", 256, 64, 128, {}, 1, True),                     # zero, subnormal, D - 1.01, random
    "fallback_d256": ("disparity_only_unary", 96, 32, 256, {}, 1, False),         # k_prepare_fused<CARRY>
}


@functools.lru_cache(maxsize=None)
def _case(name):
    preset, rows, cols, D, ov, images, hostile = SHAPES[name]
    case = helpers.build_case(preset, rows, cols, D, seed=83, n_images=images, **ov)
    if hostile:
        helpers.make_hostile(case, seed=84)
    return case


@functools.lru_cache(maxsize=None)
def _oracle_carries(name):
    """[image][column][ceil(H / 32)][D]: rows 32 k of the oracle's table (computed once per shape)."""
    case = _case(name)
    cfg, p = case["cfg"], case["params"]
    H, nb = int(cfg.rows), (int(cfg.rows) + 31) // 32
    out = []
    for img in range(len(case["frames"])):
        joined = oracle.join_columns(cfg, case["disparity"][img])
        out.append(np.stack([oracle.object_lut_column(p, joined[c], case["lut"])[:, : H + 1].T[0: 32 * nb: 32]
                             for c in range(cfg.realcols)]))
    return np.stack(out)


def _walk_carries(case, monkeypatch):
    """(carries [n * C][nb][D], outputs, lut_carry_lds) of a walk call."""
    core = _core(case, monkeypatch, dict(IS_UNARY_PATH="1"))
    try:
        out = _run(core, case, want_tables=False)
        assert core.unary_path() == (1, 0)
        n = len(case["frames"]) * case["cfg"].realcols
        return np.stack([core.read_lut_carries(c) for c in range(n)]), out, core.lut_carry_lds()[0]
    finally:
        core.close()


@pytest.mark.parametrize("name", list(SHAPES))
def test_carries_equal_the_oracle_and_the_tile_path_table(name, monkeypatch):
    case = _case(name)
    cfg = case["cfg"]
    D, C, n = int(cfg.max_dis), cfg.realcols, len(case["frames"])
    if name == "two_fn_odd_columns":
        assert n * C == 15
    got, _, on = _walk_carries(case, monkeypatch)
    assert on == (1 if D <= 128 else 0)
    want = _oracle_carries(name).reshape(got.shape)
    assert not want[:, 0].any()
    for c in range(n * C):
        assert np.array_equal(helpers.bits(want[c]), helpers.bits(got[c])), f"column {c}: not the oracle's bits"
    tile = _core(case, monkeypatch, dict(IS_UNARY_PATH="0", IS_LUT_FUSED="0"))  # (the table in the prepare launch)
    try:
        _run(tile, case, want_tables=False)
        assert tile.unary_path() == (0, 0) and tile.lut_carry_lds()[0] == 0
        nb = got.shape[1]
        for c in range(n * C):
            rows = tile.read_object_lut(c)[0: 32 * nb: 32]
            assert np.array_equal(helpers.bits(rows), helpers.bits(got[c])), f"column {c}: not the tile path's bits"
    finally:
        tile.close()


def test_more_columns_than_one_pass_of_the_grid(monkeypatch):
    base = helpers.build_case("drn_d_22_unary", 96, 512, 64, seed=89, n_images=2)
    cfg, p = base["cfg"], base["params"]
    C, H = cfg.realcols, int(cfg.rows)
    from instance_stixels_amd.core import Core
    probe = Core(base["params"], base["lut"], base["odr"], max_batch=1)
    try:
        pass_columns = probe.lut_carry_lds()[1]
    finally:
        probe.close()
    images = pass_columns // C + 1   # one image more than a pass of the grid-stride loop takes
    assert images * C > pass_columns > 0
    case = helpers.sub_case(base, [i % 2 for i in range(images)])
    got, _, on = _walk_carries(case, monkeypatch)
    assert on == 1
    nb = (H + 31) // 32
    want = []
    for img in range(2):
        joined = oracle.join_columns(cfg, base["disparity"][img])
        want.append(np.stack([oracle.object_lut_column(p, joined[c], base["lut"])[:, : H + 1].T[0: 32 * nb: 32]
                              for c in range(C)]))
    got = got.reshape(images, C, nb, -1)
    for img in range(images):
        assert np.array_equal(helpers.bits(want[img % 2]), helpers.bits(got[img])), f"image {img}"


@pytest.mark.parametrize("name", ["partial_last_block", "two_fn_odd_columns", "hostile"])
def test_walk_sections_equal_the_oracle(name, monkeypatch):
    case = _case(name)
    _, out, on = _walk_carries(case, monkeypatch)
    assert on == 1
    for img in range(len(case["frames"])):
        ref = helpers.run_oracle(case, image=img, joined=out["joined"][img])
        assert helpers.sections_equal(ref["sections"], out["sections"][img]), f"image {img}: Sections differ"


def test_tile_call_after_a_walk_call_has_complete_tables(monkeypatch):
    case = _case("two_fn_odd_columns")
    cfg, p = case["cfg"], case["params"]
    core = _core(case, monkeypatch, dict(IS_UNARY_PATH="1", IS_LUT_FUSED="0"))
    try:
        _run(core, case, want_tables=False)
        assert core.unary_path() == (1, 0) and core.lut_carry_lds()[0] == 1
        got = _run(core, case, want_tables=True)
        assert core.unary_path() == (0, 0) and core.lut_carry_lds()[0] == 0, "a call with tables takes the tile path"
        for img in range(len(case["frames"])):
            for c in range(cfg.realcols):
                want = oracle.object_lut_column(p, got["joined"][img][c], case["lut"])[:, : cfg.rows + 1]
                lut = core.read_object_lut(img * cfg.realcols + c)
                assert np.array_equal(helpers.bits(want.T), helpers.bits(lut)), (img, c)
            ref = helpers.run_oracle(case, image=img, joined=got["joined"][img])
            assert helpers.sections_equal(ref["sections"], got["sections"][img]), f"image {img}: Sections differ"
    finally:
        core.close()


def test_routing(monkeypatch):
    def route(name, env, pairwise_preset=None):
        case = _case(name)
        if pairwise_preset:
            _, rows, cols, D, ov, images, _ = SHAPES[name]
            case = helpers.build_case(pairwise_preset, rows, cols, D, seed=83, n_images=images, **ov)
        core = _core(case, monkeypatch, env)
        try:
            assert core.lut_carry_lds()[0] == -1
            if pairwise_preset:
                helpers_out = core.run(disparity_big=case["disparity"], segmentation=case["segmentation"],
                                       ground_function=case["gf"], normalization_ground=case["ng"],
                                       inv_sigma2_ground=case["ig"], vhor=case["vhor"], pairwise=True,
                                       median_join=bool(case["cfg"].median_join), want_tables=False)
                assert helpers_out is not None
                return None, core.lut_carry_lds()[0]
            _run(core, case, want_tables=False)
            return core.unary_path()[0], core.lut_carry_lds()[0]
        finally:
            core.close()

    assert route("one_block_masked_lanes", dict(IS_UNARY_PATH="1")) == (1, 1)   # D = 48
    assert route("partial_last_block", dict(IS_UNARY_PATH="1")) == (1, 1)       # D = 64
    assert route("two_fn_odd_columns", dict(IS_UNARY_PATH="1")) == (1, 1)       # D = 128
    assert route("fallback_d256", dict(IS_UNARY_PATH="1")) == (1, 0)            # D = 256: k_prepare_fused<CARRY>
    assert route("two_fn_odd_columns", dict(IS_UNARY_PATH="0")) == (0, 0)       # a tile call
    assert route("two_fn_odd_columns", {}) == (0, 0)                            # too few columns for the walk
    assert route("two_fn_odd_columns", {}, pairwise_preset="drn_d_38_pairwise") == (None, 0)
