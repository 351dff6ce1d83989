"""The prepare launch (prepare_columns_body, is_k_prepare.hip) builds the 128-byte row records, the PruneRec and the fn
windows of every column in front of every call, unary and pairwise.  How a column's records are stored and how its four
fp32 scan trees are read depends on the row count alone; with R = ceil(rows / 256) rows per thread:

  rows   what it reaches
   256   R = 1; a power of two, so the scan tree has `rows` leaves and the prefix at index `rows` is its root; row `rows`
         opens an epilogue block of its own
   264   R = 2; a tree of 512 leaves; the second epilogue block holds 9 rows
   512   R = 2; a power of two; three epilogue blocks
   520   R = 3: 256 is no multiple of it, so the instance rows of some threads straddle two epilogue blocks
  2296   R = 9: the last shape whose prefixes a thread keeps in registers
  2304   the prefixes go to the records field by field (73 KB of LDS per workgroup)

Every case is a call of 8 stixel columns and 64 disparities (fn windows on) with tables requested; Sections, cost tables
and index tables must be bit-equal to the oracle (helpers.compare).  The unary cases run on the tile path
(IS_UNARY_PATH=0), which reads every record row, so that every table row is compared: each row count; 264, 520 and 2304
with an invalid-disparity value and two images (the valid-count plane; 2304 without one is its other branch); 264 and
2304 with out-of-encoding columns (RowRecWide).  The pairwise cases (256, 520, 2304: phase 2 reads the compact disparity
and valid-count prefixes) run with the defaults and with every tile windowed (IS_P1_WIN_TILES), so that phase 1
consumes the fn windows the prepare launch chose.  No case is left out: before this file the suite had one call with R = 3
(768 rows, tests/test_parity_gpu.py, Sections only) and none above R = 4."""
import pytest

import helpers

pytestmark = pytest.mark.gpu

COLS, D = 64, 64
KNOBS = ("IS_UNARY_PATH", "IS_P1_WIN_TILES", "IS_LUT_FUSED")
# (preset, rows, images, invalid value, hostile)
UNARY, PAIRWISE = "drn_d_22_unary", "drn_d_38_pairwise"
CASES = [(UNARY, rows, 1, False, False) for rows in (256, 264, 512, 520, 2296, 2304)]
CASES += [(UNARY, rows, 2, True, False) for rows in (264, 520, 2304)]
CASES += [(UNARY, rows, 1, False, True) for rows in (264, 2304)]
CASES += [(PAIRWISE, rows, 1, False, False) for rows in (256, 520, 2304)]


def _case_id(c):
    preset, rows, n, inv, hostile = c
    return "%s-%d-%dimg%s%s" % ("pairwise" if preset == PAIRWISE else "unary", rows, n, "-invalid" if inv else "",
                                "-hostile" if hostile else "")


def _run(case, env, monkeypatch):
    from instance_stixels_amd.core import Core
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg = case["cfg"]
    core = Core(case["params"], case["lut"], case["odr"], max_batch=len(case["frames"]))   # (reads the knobs)
    try:
        return core.run(disparity_big=case["disparity"], segmentation=case["segmentation"],
                        ground_function=case["gf"], normalization_ground=case["ng"], inv_sigma2_ground=case["ig"],
                        vhor=case["vhor"], pairwise=bool(cfg.pairwise), median_join=bool(cfg.median_join),
                        want_tables=True)
    finally:
        core.close()


@pytest.mark.parametrize("c", CASES, ids=_case_id)
def test_records_of_every_store_path_give_the_oracles_tables(c, monkeypatch):
    preset, rows, n, inv, hostile = c
    ov = dict(invalid_disparity=0.0) if inv else {}
    case = helpers.build_case(preset, rows, COLS, D, seed=19, n_images=n, **ov)
    if hostile:
        case = helpers.make_hostile(case, seed=7064)
    cfg = case["cfg"]
    assert cfg.realcols == 8 and bool(cfg.pairwise) == (preset == PAIRWISE)
    refs = [helpers.run_oracle(case, image=i) for i in range(n)]          # once, for every run of the case
    if cfg.pairwise:
        runs = [("default", {}), ("all tiles windowed", {"IS_P1_WIN_TILES": str((rows + 63) // 64)})]
    else:
        runs = [("tiles", {"IS_UNARY_PATH": "0"})]
    for name, env in runs:
        got = _run(case, env, monkeypatch)
        for i in range(n):
            errs = helpers.compare(refs[i], got, i, cfg)
            assert not errs, "%s, image %d:\n" % (name, i) + "\n".join(errs[:10])
