"""k_prepare_columns (is_k_prepare.hip) is compiled for the two benchmarked row counts, 1024 and 784, beside the body that
takes its rows at run time.  Which kernel a call launches follows from the context's rows alone, so the cases are:

  rows 1024, 784                 the compiled-in shapes: five and four live epilogue blocks, a tree of 1024 leaves both
  rows 1016, 1032, 776, 792      their neighbours, on the run-time body right beside them

on the tile path with tables requested (IS_UNARY_PATH=0, which reads every record row): Sections, cost table and index
table bit-equal to the oracle (helpers.compare); 1024 and 784 also with an invalid-disparity value and two images (the
valid-count plane), with one out-of-encoding column (RowRecWide) and pairwise (S / V copies written; with the defaults
and with every tile windowed).  Every case is a call of 8 stixel columns and 64 disparities, as in
tests/test_prepare_shapes_gpu.py.

Which launch builds the records matters as much as the rows: a small tile-path call and every pairwise call take
k_prepare_fused, whose column blocks are the run-time body at any row count.  k_prepare_columns -- the kernel that is
compiled for a row count -- is launched where the LUT units run elsewhere: with them fused into the DP launch
(IS_LUT_FUSED=1, the second run of every unary tile-path case) and in a walk call (carry rows from k_lut_carry).  So the
walk runs at 1024 and 784 rows: its Sections (IS_UNARY_PATH=1), the table rows it visits (2), and the distrusted walk
(3), whose repair launches rewrite every row of every column from those records -- plain, with an invalid-disparity
value and two images, and with the out-of-encoding column.

The fn windows the prepare launch chooses cost time, not results, when they are wrong, so the last two tests count.  A
walk call (k_unary_path) reads no window; the tile path and the pairwise phase 1 do.  With every tile windowed
(IS_P1_WIN_TILES=16) a tile-path call of frame B on a context that has just run a walk call of frame A must read outside
its windows exactly as often as the same call on a fresh context -- with the records from k_prepare_fused and, LUT units
fused, from k_prepare_columns -- and so must a pairwise call behind a walk call: each call has the windows of its own
frame, whatever the call before it was.  The counts are also pinned (WINDOW_MISS; the windows and the DP kernel are the
same with and without the fused LUT units, so is the count): a library that computes no windows at all agrees with
itself on a fresh context, not with them.  (A prepare launch without
windows for walk calls was built and measured with these tests in place, and not kept: LOG.md.)"""
import functools

import numpy as np
import pytest

import helpers
import test_unary_path_gpu as walk
import test_unary_routes_gpu as routes

pytestmark = pytest.mark.gpu

COLS, D = 64, 64
KNOBS = ("IS_UNARY_PATH", "IS_P1_WIN_TILES", "IS_LUT_FUSED", "IS_NO_PRUNE")
UNARY, PAIRWISE = "drn_d_22_unary", "drn_d_38_pairwise"
COMPILED, BESIDE = (1024, 784), (1016, 1032, 776, 792)
# (preset, rows, images, invalid value, generic column)
CASES = [(UNARY, rows, 1, False, False) for rows in COMPILED + BESIDE]
CASES += [(UNARY, rows, 2, True, False) for rows in COMPILED]
CASES += [(UNARY, rows, 1, False, True) for rows in COMPILED]
CASES += [(PAIRWISE, rows, 1, False, False) for rows in COMPILED]
GENERIC_COLUMN = 5
# unary_window_miss / p1_window_miss of frame B of _two_frames() with every tile windowed, counted by the library built
# from commit 5fe802b, before k_prepare_columns was compiled for a row count
WINDOW_MISS = {UNARY: 44, PAIRWISE: 70}


def _case_id(c):
    preset, rows, n, inv, generic = c
    return "%s-%d-%dimg%s%s" % ("pairwise" if preset == PAIRWISE else "unary", rows, n, "-invalid" if inv else "",
                                "-generic" if generic else "")


@functools.lru_cache(maxsize=None)
def _case(preset, rows, n, inv, generic):
    """The case and the oracle's results of its images: once, for every test that runs it."""
    ov = dict(invalid_disparity=0.0) if inv else {}
    case = helpers.build_case(preset, rows, COLS, D, seed=19, n_images=n, **ov)
    if generic:     # a negative class value: the column leaves the FAST encodings (prep_instance_sums), it alone
        assert (case["segmentation"][:, :, :19] >= 0).all()
        case["segmentation"][:, GENERIC_COLUMN, 3, :] = -1
    cfg = case["cfg"]
    assert cfg.realcols == 8 and bool(cfg.pairwise) == (preset == PAIRWISE)
    return case, [helpers.run_oracle(case, image=i) for i in range(n)]


def _clear(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _run(core, case, want_tables):
    cfg = case["cfg"]
    return core.run(disparity_big=case["disparity"], segmentation=case["segmentation"], ground_function=case["gf"],
                    normalization_ground=case["ng"], inv_sigma2_ground=case["ig"], vhor=case["vhor"],
                    pairwise=bool(cfg.pairwise), median_join=bool(cfg.median_join), want_tables=want_tables,
                    want_instances=False)


@pytest.mark.parametrize("c", CASES, ids=_case_id)
def test_tile_path_tables_at_and_beside_the_compiled_row_counts(c, monkeypatch):
    preset, rows, n, inv, generic = c
    case, refs = _case(*c)
    cfg = case["cfg"]
    _clear(monkeypatch)
    if cfg.pairwise:
        runs = [("default", {}), ("all tiles windowed", {"IS_P1_WIN_TILES": str((rows + 63) // 64)})]
    else:
        runs = [("tiles", {"IS_UNARY_PATH": "0"}), ("tiles, LUT units fused", {"IS_UNARY_PATH": "0", "IS_LUT_FUSED": "1"})]
    for name, env in runs:
        core = walk._core(case, monkeypatch, env)
        try:
            got = _run(core, case, want_tables=True)
            state, repaired = core.unary_path(), core.lut_fused_repaired()
        finally:
            core.close()
        assert cfg.pairwise or (state[0] == 0 and repaired == 0), (name, state, repaired)
        for i in range(n):
            errs = helpers.compare(refs[i], got, i, cfg)
            assert not errs, "%s, image %d:\n" % (name, i) + "\n".join(errs[:10])


@pytest.mark.parametrize("path", ["1", "2"])
@pytest.mark.parametrize("rows", COMPILED)
def test_walk_gives_the_oracles_sections(rows, path, monkeypatch):
    case, refs = _case(UNARY, rows, 1, False, False)
    cfg = case["cfg"]
    _clear(monkeypatch)
    core = walk._core(case, monkeypatch, {"IS_UNARY_PATH": path})
    try:
        got = walk._run(core, case, want_tables=path == "2", prefill=True)
        state = core.unary_path()
    finally:
        core.close()
    assert state == (1, 0), state      # the walk ran and trusted itself
    errs = helpers.compare(refs[0], got, 0, cfg, check_tables=False)
    if path == "2":
        errs += routes._visited_rows_match(refs[0], got, 0, cfg)
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("c", [c for c in CASES if c[0] == UNARY and c[1] in COMPILED], ids=_case_id)
def test_distrusted_walk_repairs_every_column(c, monkeypatch):
    case, refs = _case(*c)
    cfg = case["cfg"]
    _clear(monkeypatch)
    core = walk._core(case, monkeypatch, {"IS_UNARY_PATH": "3"})
    try:
        got = walk._run(core, case, want_tables=True, prefill=True)
        state = core.unary_path()
    finally:
        core.close()
    assert state == (1, 1), state      # the walk ran, distrusted itself, and the repair launches rewrote the call
    got["cost_table"] = got["cost_bits"].view(np.float32)
    for i in range(len(refs)):
        errs = helpers.compare(refs[i], got, i, cfg) + routes._initial_indices_match(refs[i], got, i, cfg)
        assert not errs, "image %d:\n" % i + "\n".join(errs[:10])


@functools.lru_cache(maxsize=None)
def _two_frames(preset):
    """Frames A and B of one configuration, and the oracle's results for B."""
    case2 = helpers.build_case(preset, 1024, COLS, D, seed=43, n_images=2)
    a, b = helpers.sub_case(case2, [0]), helpers.sub_case(case2, [1])
    assert not np.array_equal(a["disparity"], b["disparity"])
    return a, b, helpers.run_oracle(b, image=0)


def _window_misses_of_b(preset, fused, walk_first, monkeypatch):
    a, b, ref_b = _two_frames(preset)
    cfg = b["cfg"]
    _clear(monkeypatch)
    env = {"IS_UNARY_PATH": "1", "IS_P1_WIN_TILES": "16"}
    if fused:
        env["IS_LUT_FUSED"] = "1"
    core = walk._core(b, monkeypatch, env)
    try:
        if walk_first:
            got_a = walk._run(core, a, want_tables=False)     # (a unary call, whatever the preset)
            assert core.unary_path() == (1, 0), core.unary_path()
            assert got_a["sections"].shape[1] == cfg.realcols
        core.set_eval_counters(True)     # (zeroes them; a counting unary call takes the tile path)
        got = _run(core, b, want_tables=False)
        counters = core.eval_counters()
        assert cfg.pairwise or (core.unary_path()[0] == 0 and core.lut_fused_repaired() == 0)
    finally:
        core.close()
    errs = helpers.compare(ref_b, got, 0, cfg, check_tables=False)
    assert not errs, "\n".join(errs[:10])
    return int(counters["p1_window_miss" if cfg.pairwise else "unary_window_miss"])


@pytest.mark.parametrize("preset,fused", [(UNARY, False), (UNARY, True), (PAIRWISE, False)],
                         ids=["unary", "unary-lut-fused", "pairwise"])
def test_windows_are_computed_for_the_call_behind_a_walk_call(preset, fused, monkeypatch):
    fresh = _window_misses_of_b(preset, fused, False, monkeypatch)
    behind = _window_misses_of_b(preset, fused, True, monkeypatch)
    print("window misses of frame B (%s%s): fresh context %d, behind a walk call of frame A %d"
          % (preset, ", LUT units fused" if fused else "", fresh, behind))
    assert preset == PAIRWISE or fresh > 0
    assert behind == fresh
    assert fresh == WINDOW_MISS[preset]
