"""Phase 1 of the pairwise DP (k_pw_phase1, is_k_pairwise.hip) runs, per (column, tile): the tile-0 shortcut, or staging
with the summary prefetch, the L7 / L8 pre-pass, the FAST descending walk (full steps, ground / sky rounds, the L7
skip) or the generic ascending walk, the first segment, the wave merge -- in six instantiations (with / without an
invalid-disparity value x the whole lutT row in registers, D <= 128 / the per-lane gather, D > 128 / the fn window).
Small calls through every route of that code:

  (a) Sections, cost tables and index tables bit-equal to the oracle (helpers.compare);
  (b) the evaluation counters of phase 1 -- full steps, ground / sky candidates, steps with a lane outside the fn
      window -- equal to the values the library of commit 60344e0 counted for the same case (EXPECTED).  Parity
      alone does not see a pruning change that keeps the results exact.

Shapes, the smallest at which each route exists: rows = 160 (tiles of 64, 64 and 32 rows) and 136 (a last tile of 8
rows: dead lanes in every ballot), 48 or 64 image columns; D = 64 classic (IS_P1_WIN_TILES=0, <., 2>) and windowed
(IS_P1_WIN_TILES=99, <., 2, true>), D = 160 (<., 0>); with and without invalid_disparity; one hostile case per D = 64
route (generic columns, the ascending walk, beside FAST ones; windowed: lanes outside the window, the counter is
asserted non-zero); the horizon at row 0 (every tile NOGROUND, everything is sky range), inside the middle tile (a sky
range, then a ground range) and at rows - 1 (no sky range); one and two images (nsplit = 2) and three images of 172
columns (516 > IS_PW_SPLIT_MAX_COLS columns: nsplit = 1); IS_NO_PRUNE=1 (L7 off, no type ever closes, every wave that
owns vB = 0 reaches the first segment); and 2112 rows x 2 columns x 32 disparities: 33 tiles, the last with 65 > 63
bound blocks (L7 off by the block count; its phase-1 launch asks for 47 KB of LDS, the oracle takes under a second)."""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

PRESET = "drn_d_38_pairwise"
KNOBS = ("IS_P1_WIN_TILES", "IS_NO_PRUNE")
CLASSIC, WINDOWED = {"IS_P1_WIN_TILES": "0"}, {"IS_P1_WIN_TILES": "99"}

# id: (rows, image columns, D, images, invalid value, hostile seed or None, horizon or None, knobs)
CASES = {
    "160-classic": (160, 48, 64, 1, False, None, None, CLASSIC),
    "160-classic-2img-invalid": (160, 48, 64, 2, True, None, None, CLASSIC),
    "136-classic-invalid": (136, 48, 64, 1, True, None, None, CLASSIC),
    "160-windowed-invalid": (160, 48, 64, 1, True, None, None, WINDOWED),
    "136-windowed-2img": (136, 48, 64, 2, False, None, None, WINDOWED),
    "160-classic-hostile": (160, 64, 64, 2, False, 7064, None, CLASSIC),
    "160-windowed-hostile": (160, 64, 64, 2, False, 7064, None, WINDOWED),
    "136-d160": (136, 48, 160, 1, False, None, None, CLASSIC),
    "160-d160-invalid": (160, 48, 160, 1, True, None, None, CLASSIC),
    "160-classic-horizon0": (160, 48, 64, 1, False, None, 0, CLASSIC),
    "160-windowed-horizon0": (160, 48, 64, 1, False, None, 0, WINDOWED),
    "160-classic-horizon100": (160, 48, 64, 1, False, None, 100, CLASSIC),
    "160-windowed-horizon100": (160, 48, 64, 1, False, None, 100, WINDOWED),
    "160-classic-horizon159": (160, 48, 64, 1, False, None, 159, CLASSIC),
    "160-windowed-horizon159": (160, 48, 64, 1, False, None, 159, WINDOWED),
    "136-windowed-3img-nsplit1": (136, 1376, 64, 3, False, None, None, WINDOWED),
    "160-classic-noprune": (160, 48, 64, 1, False, None, None, dict(CLASSIC, IS_NO_PRUNE="1")),
    "2112-d32-65blocks": (2112, 16, 32, 1, False, None, None, {}),
}

# (p1_full, p1_gs, p1_window_miss) of each case, counted by the library built from commit 60344e0
EXPECTED = {
    "160-classic": (507, 10, 0),
    "160-classic-2img-invalid": (959, 14, 0),
    "136-classic-invalid": (458, 55, 0),
    "160-windowed-invalid": (371, 35, 62),
    "136-windowed-2img": (641, 182, 41),
    "160-classic-hostile": (1064, 9, 0),
    "160-windowed-hostile": (847, 96, 146),
    "136-d160": (445, 55, 0),
    "160-d160-invalid": (497, 18, 0),
    "160-classic-horizon0": (631, 128, 0),
    "160-windowed-horizon0": (492, 140, 100),
    "160-classic-horizon100": (508, 0, 0),
    "160-windowed-horizon100": (367, 7, 80),
    "160-classic-horizon159": (1170, 0, 0),
    "160-windowed-horizon159": (1170, 0, 181),
    "136-windowed-3img-nsplit1": (22746, 2907, 1151),
    "160-classic-noprune": (1170, 0, 0),
    "2112-d32-65blocks": (44905, 1051, 0),
}


@pytest.mark.parametrize("name", list(CASES))
def test_phase1_routes_agree_with_the_oracle_and_count_the_parents_steps(name, monkeypatch):
    from instance_stixels_amd.core import Core
    rows, cols, D, n, inv, hostile, vhor, env = CASES[name]
    ov = dict(invalid_disparity=0.0) if inv else {}
    case = helpers.build_case(PRESET, rows, cols, D, seed=11, n_images=n, **ov)
    if hostile is not None:
        case = helpers.make_hostile(case, seed=hostile)
    if vhor is not None:
        case["vhor"][:] = vhor        # (the oracle and the core both take the horizon from the case)
    cfg = case["cfg"]
    assert (n * cfg.realcols > 512) == name.endswith("nsplit1")           # IS_PW_SPLIT_MAX_COLS
    refs = [helpers.run_oracle(case, image=i) for i in range(n)]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    core = Core(case["params"], case["lut"], case["odr"], max_batch=n)   # (reads the knobs)
    try:
        core.set_eval_counters(True)
        got = core.run(disparity_big=case["disparity"], segmentation=case["segmentation"],
                       ground_function=case["gf"], normalization_ground=case["ng"],
                       inv_sigma2_ground=case["ig"], vhor=case["vhor"], pairwise=True,
                       median_join=bool(cfg.median_join), want_tables=True)
        cnt = core.eval_counters()
        if hostile is not None:
            never = np.array([bool(np.all(core.read_block_summaries(c)[1, :3] == -np.inf))
                              for c in range(n * cfg.realcols)])
    finally:
        core.close()
    counted = (cnt["p1_full"], cnt["p1_gs"], cnt["p1_window_miss"])
    for i in range(n):                                                    # (a)
        errs = helpers.compare(refs[i], got, i, cfg)
        assert not errs, "image %d:\n" % i + "\n".join(errs[:10])
    if hostile is not None:   # generic columns (their block summaries never bound: -inf) beside FAST ones
        assert never.any() and not never.all(), never.tolist()
    if name == "160-windowed-hostile":
        assert counted[2] > 0, "no lane read outside its fn window"
    if env.get("IS_P1_WIN_TILES") == "0":
        assert counted[2] == 0
    assert counted == EXPECTED[name]                                      # (b)
