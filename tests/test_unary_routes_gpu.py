"""The unary DP evaluates a segment (vB, vT) in three kernels -- k_dp_unary (tile pairs), k_dp_unary_fast (ring and
windows) and k_unary_path (the walk) -- around ONE copy of what they share (is_unary.h: the cost, the update of the
bests with its `<` / `<=`, live / FIRST / NOGROUND forms, the merge's tie rule, the final index of a row without a finite
candidate, the merge and row store of the tile kernels).  The same small calls go through every route, each with
tables requested; Sections, cost tables and index tables must be bit-equal to the oracle (helpers.compare), for the
walk at the rows it visits (as tests/test_unary_path_gpu.py does it; the rows it does not visit keep their pattern).

Routes: the windowed ring kernel (IS_UNARY_PATH=0), the same with the LUT units fused into the launch (IS_LUT_FUSED=1),
the classic 8-wave tiles (IS_P1_WIN_TILES=0), the walk (IS_UNARY_PATH=2), and the walk distrusted, so that the gated
k_dp_unary<.., true, true> rewrites every FAST column (IS_UNARY_PATH=3).

Shapes, the smallest at which the shared pieces meet their edges: 160 rows (tiles of 64, 64 and 32) and 136 (H % 64
!= 0, a last tile of 8 rows), 8 stixel columns, 64 disparities (windowed); one image, and two with different horizons
(87 or 74: the middle tile holds it and the last lies wholly above it, NOGROUND; 39 in the second image: the first tile
holds it); with and without an invalid-disparity value; one hostile case, whose generic columns go through the
ascending `<` form; one call of 320 disparities: above 256 there is no ring kernel and k_dp_unary<.., true> is the
primary route of the FAST columns; and one of 196 disparities with an invalid-disparity value through the three tile
routes: the smallest count with four fn blocks that is windowed, where k_dp_unary_fast<true, 4> runs classic, windowed
and with the LUT units fused (and its repair launch behind them) -- instantiations no other test launches."""
import itertools

import numpy as np
import pytest

import helpers
import test_unary_path_gpu as walk

pytestmark = pytest.mark.gpu

PRESET, COLS = "drn_d_22_unary", 64
KNOBS = ("IS_UNARY_PATH", "IS_LUT_FUSED", "IS_P1_WIN_TILES")
TILE = {"IS_UNARY_PATH": "0"}
ROUTES = [("windowed", TILE),
          ("fused", dict(TILE, IS_LUT_FUSED="1")),
          ("classic", dict(TILE, IS_P1_WIN_TILES="0")),
          ("walk", {"IS_UNARY_PATH": "2"}),
          ("distrusted-walk", {"IS_UNARY_PATH": "3"})]
# (rows, max_dis, images, invalid value, hostile, routes)
CASES = [(rows, 64, n, inv, False, ROUTES)
         for rows, n, inv in itertools.product((160, 136), (1, 2), (False, True))]
CASES.append((160, 64, 2, False, True, ROUTES))       # generic columns beside FAST ones
CASES.append((136, 320, 1, False, False, ROUTES[:1]))   # D > 256: k_dp_unary<.., true> takes the FAST columns
CASES.append((136, 196, 1, True, False, ROUTES[:3]))    # k_dp_unary_fast<true, 4, ...>: windowed, fused + repair, classic


def _case_id(c):
    rows, D, n, inv, hostile, routes = c
    return "%dx%d-%dimg%s%s" % (rows, D, n, "-invalid" if inv else "", "-hostile" if hostile else "")


def _second_horizon(case, vhor):
    """Image 1 of the case with the horizon at DP row `vhor` (its ground model follows)."""
    from oracle import oracle
    cfg, f = case["cfg"], case["frames"][1]
    g = oracle.host_ground(cfg, int(cfg.rows) - 1 - vhor, f.camera_tilt, f.camera_height, f.alpha_ground)
    case["gf"][1], case["ng"][1], case["ig"][1], case["vhor"][1] = g
    assert case["vhor"][1] == vhor


def _visited_rows_match(ref, got, img, cfg):
    """The walk's tables against the oracle's: every row k_backtrace visits, and nothing else written."""
    H = int(cfg.rows)
    errs = []
    for c in range(cfg.realcols):
        mask = np.zeros(H, bool)
        mask[walk._visited(got["sections"][img][c], H)] = True
        gc, gi = got["cost_bits"][img, c], got["index_table"][img, c]
        rc, ri = helpers.bits(ref["cost_table"][c]), ref["index_table"][c]
        if not (gi[~mask] == walk.FILL_INDEX).any():    # a generic column: k_dp_unary fills every row
            mask[:] = True
        elif not ((gc[~mask] == walk.FILL_COST).all() and (gi[~mask] == walk.FILL_INDEX).all()):
            errs.append(f"col {c}: a row the back-trace does not visit was written")
        if not np.array_equal(gc[mask], rc[mask]):
            errs.append(f"col {c}: visited costs differ in rows {np.argwhere((gc != rc).any(axis=1) & mask)[:5, 0].tolist()}")
        badi = (_oracle_vb(ri) != gi) & mask[:, None]
        if badi.any():
            errs.append(f"col {c}: visited indices differ at {np.argwhere(badi)[:5].tolist()}")
    return errs


def _oracle_vb(ri):
    """The oracle's index (3 vB + predecessor type; -1: no candidate; the object type starts as OBJECT at vB = 0) as
    the winning vB the unary core stores, the initial indices -1 / 0 included."""
    return np.where(ri >= 0, ri // 3, -1)


def _initial_indices_match(ref, got, img, cfg):
    """helpers.compare looks at the indices the oracle wrote; a row without a finite candidate keeps its initial index
    (unary_final_index: -1, or 0 for the object type), and that is compared here, on every row of every column."""
    bad = _oracle_vb(ref["index_table"][:cfg.realcols]) != got["index_table"][img]
    return [f"index_table differs in {int(bad.sum())} entries, initial ones included, first {np.argwhere(bad)[:5].tolist()}"] if bad.any() else []


@pytest.mark.parametrize("c", CASES, ids=_case_id)
def test_every_unary_route_is_bit_equal_to_the_oracle(c, monkeypatch):
    rows, D, n, inv, hostile, routes = c
    ov = dict(invalid_disparity=0.0) if inv else {}
    case = helpers.build_case(PRESET, rows, COLS, D, seed=11, n_images=n, **ov)
    if n == 2:
        _second_horizon(case, 39)
    if hostile:
        case = helpers.make_hostile(case, seed=7064)
    cfg = case["cfg"]
    # one tile holds the horizon of image 0 and the last one lies wholly above it
    assert 64 <= case["vhor"][0] < (rows - 1) // 64 * 64
    refs = [helpers.run_oracle(case, image=i) for i in range(n)]          # once, for all routes
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for name, env in routes:
        core = walk._core(case, monkeypatch, env)
        try:
            got = walk._run(core, case, want_tables=True, prefill=True)
            state = core.unary_path()
        finally:
            core.close()
        expect = {"walk": (1, 0), "distrusted-walk": (1, 1)}.get(name)
        assert (state == expect) if expect else (state[0] == 0), (name, state)
        got["cost_table"] = got["cost_bits"].view(np.float32)
        for i in range(n):
            errs = helpers.compare(refs[i], got, i, cfg, check_tables=name != "walk")
            errs += _visited_rows_match(refs[i], got, i, cfg) if name == "walk" else _initial_indices_match(refs[i], got, i, cfg)
            assert not errs, name + ", image %d:\n" % i + "\n".join(errs[:10])
        if hostile and name == "walk":    # generic columns beside FAST ones: some columns are complete, some are not
            full = [not (got["index_table"][i, col] == walk.FILL_INDEX).any() for i in range(n) for col in range(cfg.realcols)]
            assert any(full) and not all(full), full
