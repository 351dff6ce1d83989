"""Phase 2 of the pairwise DP exists as three walks -- k_pw_phase2s (chain + evaluator waves, the default of
small calls), k_pw_phase2x + k_pw_phase2_generic (two columns per wave, IS_P2_SPLIT=0) and k_pw_phase2 (one
column per wave, IS_P2_SPLIT=0 IS_P2X=0, or an odd number of columns per image) -- around ONE copy of what
they share (the fn window, its staging, the merge of phase 1's minima, the object data term, the tail of
"row r is final", the table stores, the block summaries; is_k_pairwise.hip, "what the three phase-2 walks
share").  Shapes at which every shared piece meets its edge cases, through each route:

  (a) Sections, cost tables and index tables bit-equal to the oracle (as tests/test_parity_gpu.py);
  (b) per column, the block summaries the walk leaves behind (lemmas L7 / L8: from the StepRecs and T8 values
      stored when a row became final) are the same bits on all three routes.  No parity test sees that path
      except through pruning.

rows = 160: tiles of 64, 64 and 32 rows (the last: the early exit of the two-column walk, clamped rows in every
helper); rows = 136: a last tile of 8 rows, H % 64 != 0; an even and an odd number of columns per image (odd:
the planner takes k_pw_phase2 under IS_P2_SPLIT=0); with and without an invalid-disparity value; one and two
images; one case with out-of-encoding columns, whose pairs go to k_pw_phase2_generic beside FAST pairs."""
import itertools

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

PRESET, D, QB = "drn_d_38_pairwise", 32, 32
ROUTES = [("default", {}),
          ("two-column", {"IS_P2_SPLIT": "0"}),
          ("one-column", {"IS_P2_SPLIT": "0", "IS_P2X": "0"})]
CASES = [(rows, cols, n, inv, False)
         for rows, cols, n, inv in itertools.product((160, 136), (48, 40), (1, 2), (False, True))]
CASES.append((160, 64, 2, False, True))     # hostile: generic columns beside FAST ones


def _case_id(c):
    rows, cols, n, inv, hostile = c
    return "%dx%d-%dimg%s%s" % (rows, cols, n, "-invalid" if inv else "", "-hostile" if hostile else "")


def _run_route(case, env, monkeypatch):
    """-> (the call's outputs, [ncols][n_blocks][24] block summaries) under the routing knobs `env`."""
    from instance_stixels_amd.core import Core
    for k in ("IS_P2_SPLIT", "IS_P2X"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg, n = case["cfg"], len(case["frames"])
    core = Core(case["params"], case["lut"], case["odr"], max_batch=n)   # (reads the knobs)
    try:
        out = core.run(disparity_big=case["disparity"], segmentation=case["segmentation"],
                       ground_function=case["gf"], normalization_ground=case["ng"],
                       inv_sigma2_ground=case["ig"], vhor=case["vhor"], pairwise=True,
                       median_join=bool(cfg.median_join), want_tables=True)
        summ = np.stack([core.read_block_summaries(c) for c in range(n * cfg.realcols)])
    finally:
        core.close()
    return out, summ


@pytest.mark.parametrize("c", CASES, ids=_case_id)
def test_phase2_routes_agree_with_the_oracle_and_in_their_block_summaries(c, monkeypatch):
    rows, cols, n, inv, hostile = c
    ov = dict(invalid_disparity=0.0) if inv else {}
    case = helpers.build_case(PRESET, rows, cols, D, seed=11, n_images=n, **ov)
    if hostile:
        case = helpers.make_hostile(case, seed=7064)
    cfg = case["cfg"]
    assert (cfg.realcols % 2 == 1) == (cols == 40)
    refs = [helpers.run_oracle(case, image=i) for i in range(n)]          # once, for all three routes
    # the bound blocks that hold a candidate row 1 <= vB <= rows - 1 (block 0 is the first segment: phase 2 leaves none)
    n_blk = (rows - 1 + QB - 1) // QB
    first = None
    for name, env in ROUTES:
        got, summ = _run_route(case, env, monkeypatch)
        for i in range(n):                                                # (a)
            errs = helpers.compare(refs[i], got, i, cfg)
            assert not errs, name + ":\n" + "\n".join(errs[:10])
        sb = helpers.bits(summ[:, 1:n_blk + 1])                           # (b)
        if first is None:
            first = sb
            if hostile:   # generic columns carry the summaries that never bound (-inf), FAST ones real minima
                never = np.all(summ[:, 1, :3] == -np.inf, axis=1)
                pairs = never.reshape(-1, 2)
                assert (pairs.sum(axis=1) == 0).any() and (pairs.sum(axis=1) > 0).any(), never.tolist()
        else:
            bad = np.argwhere(sb != first)
            assert bad.size == 0, "%s: %d summary words differ from the default route, first (column, block - 1, float): %s" % (
                name, len(bad), bad[:8].tolist())
