"""GPU tests of what only the walk's merge of a row decides (unary_merge_lanes, is_k_unary_path.hip).

At the end of a row the 64 lanes of k_unary_path hold a partial minimum (cost, vB) per type; the merge reduces them to
the row's three costs and indices by the rule of unary_merge_take (is_unary.h): the minimum cost, among equal costs the
smallest recorded vB, and the initial index where no candidate is finite.  The tile path evaluates the same rule over
other partitions of the candidates, so it is the reference.  Every case is a small call (8 or 12 stixel columns) run
three ways into zero-filled Section buffers:
  * the tile path (IS_UNARY_PATH=0, tables and instance outputs requested);
  * the walk in its table-writing form (IS_UNARY_PATH=2, the same outputs, tables pre-filled with a NaN pattern);
  * the walk as the benchmark runs it (IS_UNARY_PATH=1, neither tables nor instance outputs: it writes the Sections).
Bit for bit: the three costs and indices of the visited rows, the pattern in every other row, and the Section
buffers of both walk forms as whole arrays.

The groups: exact cost ties across lanes (established on the CPU from every candidate's cost,
tests/independent_evaluator.py, before a device result is looked at), a type without a finite candidate (rows at or
above the horizon, row 0), a partial last block (H % 64 != 0) and the distrust path behind the merge."""
import functools

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

FILL_COST = np.uint32(0x7FC0BEEF)  # a quiet NaN no kernel writes
FILL_INDEX = np.int32(-777)
INF_BITS = np.uint32(0x7F800000)
GROUND, OBJECT, SKY = 0, 1, 2


def _core(case, monkeypatch, mode):
    from instance_stixels_amd.core import Core
    monkeypatch.setenv("IS_UNARY_PATH", mode)
    try:
        return Core(case["params"], case["lut"], case["odr"], max_batch=len(case["frames"]))
    finally:
        monkeypatch.delenv("IS_UNARY_PATH")


def _run(core, case, full):
    """One unary call into zero-filled Sections; full: with pattern-filled tables and instance outputs."""
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
    sections = torch.zeros((n, C, S, 8), dtype=torch.int32, device=dev)
    cost = index = inst = None
    if full:
        cost = torch.full((n, C, H, 3), int(FILL_COST.view(np.int32)), dtype=torch.int32, device=dev)
        index = torch.full((n, C, H, 3), int(FILL_INDEX), dtype=torch.int32, device=dev)
        com = torch.zeros((n, INSTANCE_CLASSES, C * S, 2), dtype=torch.float32, device=dev)
        idx = torch.zeros((n, INSTANCE_CLASSES, C * S, 2), dtype=torch.int32, device=dev)
        cor = torch.zeros((n, INSTANCE_CLASSES, C * S), dtype=torch.uint8, device=dev)
        per = torch.zeros((n, INSTANCE_CLASSES), dtype=torch.int32, device=dev)
        inst = [InstanceBuffers(com[i].data_ptr(), idx[i].data_ptr(), cor[i].data_ptr(), per[i].data_ptr(), None,
                                None) for i in range(n)]
    core.compute_ptr(joined.data_ptr(), seg.data_ptr(), case["gf"], case["ng"], case["ig"], case["vhor"], False, n,
                     sections.data_ptr(), inst, cost.data_ptr() if full else None, index.data_ptr() if full else None,
                     stream)
    torch.cuda.synchronize(dev)
    out = dict(raw=sections.cpu().numpy())
    out["sections"] = out["raw"].view(SECTION_DTYPE).reshape(n, C, S)
    if full:
        out["cost_bits"] = cost.cpu().numpy().view(np.uint32)
        out["index_table"] = index.cpu().numpy()
    return out


def _visited(sec_col, H):
    """The rows k_backtrace reads in a unary column: H - 1, and vB - 1 of every Section with vB > 0."""
    n = helpers.n_sections(sec_col)
    return sorted({H - 1} | {int(v) - 1 for v in sec_col["vB"][:n] if v > 0})


def _three_ways(case, monkeypatch, walk_modes=(("2", 0), ("1", 0))):
    """-> (tile output, table-form walk output).  walk_modes: (IS_UNARY_PATH of the table form, repaired calls
    expected), the same for the Section-writing form."""
    core = _core(case, monkeypatch, "0")
    try:
        tile = _run(core, case, full=True)
        assert core.unary_path()[0] == 0
    finally:
        core.close()
    outs = []
    for (mode, repaired), full in zip(walk_modes, (True, False)):
        core = _core(case, monkeypatch, mode)
        try:
            outs.append(_run(core, case, full=full))
            assert core.unary_path() == (1, repaired)
        finally:
            core.close()
    path, bare = outs
    for name, got in (("table form", path), ("Section form", bare)):
        diff = np.argwhere((got["raw"] != tile["raw"]).any(axis=(2, 3)))
        assert diff.size == 0, f"{name}: Sections differ from the tile path in (image, column) {diff[:8].tolist()}"
    return tile, path


def _check_visited(case, tile, path):
    H = int(case["cfg"].rows)
    n, C = path["index_table"].shape[:2]
    for img in range(n):
        for c in range(C):
            mask = np.zeros(H, bool)
            mask[_visited(tile["sections"][img][c], H)] = True
            pc, tc = path["cost_bits"][img, c], tile["cost_bits"][img, c]
            pi, ti = path["index_table"][img, c], tile["index_table"][img, c]
            bad = np.argwhere(mask[:, None] & ((pc != tc) | (pi != ti)))
            assert bad.size == 0, (f"image {img} column {c}: (row, type) {bad[:6].tolist()} walk "
                                   f"{[(hex(pc[r, t]), int(pi[r, t])) for r, t in bad[:6]]} tile "
                                   f"{[(hex(tc[r, t]), int(ti[r, t])) for r, t in bad[:6]]}")
            assert (pc[~mask] == FILL_COST).all() and (pi[~mask] == FILL_INDEX).all(), \
                f"image {img} column {c}: a row the back-trace does not visit was written"


def _check(case, monkeypatch):
    tile, path = _three_ways(case, monkeypatch)
    _check_visited(case, tile, path)
    return tile, path


# ---- 1. exact ties across lanes -----------------------------------------------------------------------------------
# (rows, image columns, D, seed, dw, pw, iw, invalid_disparity or None): the `ties` construction of
# test_parity_gpu._adversarial_case, restated with explicit weights.  8 or 12 stixel columns.
# Exact ties need dw = pw = 0 (a data or prior term differs for every vB); the other weights give near-ties.
TIES = [
    (128, 64, 16, 1, 0.0, 0.0, 0.0, None),
    (136, 96, 32, 2, 1e-7, 1e-6, 1e-3, 0.0),
    (192, 64, 32, 3, 0.0, 0.0, 1e-3, 0.0),
    (256, 96, 16, 4, 1e-3, 1.0, 0.0, None),
    (256, 96, 16, 4, 0.0, 0.0, 0.0, 0.0),
]
TIE_COLUMNS = (0, 1, 2, 3)  # the columns the CPU looks at: all-0, all-1, the two regions and a random one


@functools.lru_cache(maxsize=None)
def _ties_case(rows, cols, D, seed, dw, pw, iw, inv):
    ov = dict(disparity_weight=dw, prior_weight=pw, segmentation_weight=1.0, instance_weight=iw)
    if inv is not None:
        ov["invalid_disparity"] = inv
    case = helpers.build_case("drn_d_22_unary", rows, cols, D, seed=52000 + seed, **ov)
    rng = np.random.default_rng(53000 + seed)
    seg, disp = case["segmentation"], case["disparity"]
    Hs = rows // 8
    # tiny integer class values, 70 % zeros: the class-group minima move in steps of sw and meet exactly
    seg[:, :, :19, :Hs] = rng.integers(0, 3, seg[:, :, :19, :Hs].shape) * (rng.random(seg[:, :, :19, :Hs].shape) < 0.3)
    seg[:, 0, :19, :Hs] = 0                        # a column where every class ties everywhere
    seg[:, 1, :19, :Hs] = 1
    # ... and a column of two such regions, road below an object, split below the horizon: the back-trace hops to row
    # split - 1, where every ground candidate vB = 0 .. split - 1 ties (the other columns' visited rows below the
    # horizon are few)
    ks = min(int(case["vhor"][0]), rows - 8) // 8
    seg[:, 2, :19, :Hs] = 2
    seg[:, 2, 0, :ks] = 0
    seg[:, 2, 13, ks:Hs] = 0
    seg[:, :, 19:, :Hs] = rng.integers(-2, 3, seg[:, :, 19:, :Hs].shape)
    disp[:] = np.float32(3.5)                      # constant data terms
    return case


@functools.lru_cache(maxsize=None)
def _merge_ties(spec):
    """What the merge has to decide in a ties case, from every candidate's cost on the CPU: per type the number of
    visited rows whose minimum is attained by candidates of different lanes (lane of vB: (vB - 1) mod 64, vB = 0 in
    lane 0), how many of these have tied candidates in different 64-row blocks (different steps of the walk), and how
    many are won by vB = 0."""
    import independent_evaluator as ie
    from oracle import oracle
    case = _ties_case(*spec)
    cfg, p = case["cfg"], case["params"]
    F32 = np.float32
    H, vhor = int(cfg.rows), int(case["vhor"][0])
    joined = oracle.join_columns(cfg, case["disparity"][0])
    lanes_differ = {GROUND: 0, OBJECT: 0, SKY: 0}
    blocks_differ = first_wins = 0
    for c in TIE_COLUMNS:
        tr = {}
        ct, it, secs = ie.evaluate_column(p, c, joined[c], case["segmentation"][0][c], case["gf"][0].astype(F32),
                                          case["ng"][0].astype(F32), case["ig"][0].astype(F32), vhor,
                                          np.asarray(case["lut"], F32), np.asarray(case["odr"], F32), False, trace=tr)
        rows = sorted({H - 1} | {int(s[1]) - 1 for s in secs if s[1] > 0})
        for vT in rows:
            for typ in (GROUND, OBJECT, SKY):
                m = ct[vT, typ]
                if not np.isfinite(m):
                    continue
                tied = []
                for b in range(1, vT + 1):
                    t_b, _, cgs, cob = tr["pair"][b]
                    if typ == OBJECT:
                        cost = cob[vT - b]
                    elif typ == t_b:
                        cost = cgs[vT - b]
                    else:
                        continue
                    if cost == m:
                        tied.append(b)
                winner = int(it[vT, typ]) // 3
                if winner == 0:                    # (strict <, ascending vB: the first segment attains m iff it won)
                    tied.insert(0, 0)
                assert tied and tied[0] == winner, (c, vT, typ, winner, tied[:4])
                if len({(b - 1) % 64 if b else 0 for b in tied}) < 2:
                    continue
                lanes_differ[typ] += 1
                blocks_differ += len({(b - 1) // 64 for b in tied if b}) > 1
                first_wins += winner == 0
    return lanes_differ, blocks_differ, first_wins


@functools.lru_cache(maxsize=None)
def _the_fixture_set_has_merge_ties():
    """Asserted before the device results of any ties case are looked at: over the set, for each type a visited row
    with a tie across lanes, one with a tie across 64-row blocks, one that vB = 0 wins."""
    total = {GROUND: 0, OBJECT: 0, SKY: 0}
    blocks = first = 0
    for spec in TIES:
        lanes_differ, b, f = _merge_ties(spec)
        for typ in total:
            total[typ] += lanes_differ[typ]
        blocks += b
        first += f
    print("visited rows with a tie across lanes (ground, object, sky):", total, "| across blocks:", blocks,
          "| won by vB = 0:", first)
    assert all(v > 0 for v in total.values()), total
    assert blocks > 0 and first > 0, (blocks, first)
    return True


@pytest.mark.parametrize("spec", TIES, ids=[f"{s[0]}x{s[1]}x{s[2]}-{i}" for i, s in enumerate(TIES)])
def test_ties_across_lanes_take_the_smallest_vB(spec, monkeypatch):
    assert _the_fixture_set_has_merge_ties()
    _check(_ties_case(*spec), monkeypatch)


# ---- 2. a type without a finite candidate ----------------------------------------------------------------------------
def _horizon_case(rows, cols, D, seed, horizons, **ov):
    """The `horizon_in_tile` construction: one image per horizon row, the ground model rebuilt for it."""
    from oracle import oracle
    case = helpers.build_case("drn_d_22_unary", rows, cols, D, seed=seed, n_images=len(horizons), **ov)
    for i, (f, vh) in enumerate(zip(case["frames"], horizons)):
        g = oracle.host_ground(case["cfg"], int(vh), f.camera_tilt, f.camera_height, f.alpha_ground)
        case["gf"][i], case["ng"][i], case["ig"][i], case["vhor"][i] = g
    return case


@pytest.mark.parametrize("inv", [None, 0.0], ids=["all_valid", "invalid_0"])
def test_rows_above_the_horizon_have_no_ground_candidate(inv, monkeypatch):
    rows = 192
    ov = {} if inv is None else dict(invalid_disparity=inv)
    case = _horizon_case(rows, 64, 32, 61, (1, 63, 64, 65, rows - 2), **ov)
    tile, path = _check(case, monkeypatch)
    checked = 0
    for img in range(len(case["frames"])):
        vhor = int(case["vhor"][img])
        for c in range(path["index_table"].shape[1]):
            for vT in _visited(tile["sections"][img][c], rows):
                if vT >= vhor:                     # the ground data prefix is +inf from row vhor on, in every lane
                    assert path["cost_bits"][img, c, vT, GROUND] == INF_BITS, (img, c, vT)
                    assert path["index_table"][img, c, vT, GROUND] == -1, (img, c, vT)
                    checked += 1
    assert checked >= len(case["frames"]), "no visited row at or above a horizon"


def test_row_0_has_the_first_segment_only(monkeypatch):
    """Without the prior term a shorter segment is never dearer: the back-trace hops row by row down to row 0, where
    vB = 0 is the only candidate and 63 lanes hold the initial pair for every type."""
    rows = 128
    case = helpers.build_case("drn_d_22_unary", rows, 64, 32, seed=67, n_images=2, prior_weight=0.0)
    tile, path = _check(case, monkeypatch)
    cols = [(img, c) for img in range(2) for c in range(path["index_table"].shape[1])
            if 0 in _visited(tile["sections"][img][c], rows)]
    assert cols, "row 0 is visited in no column: the case does not reach vT = 0"
    for img, c in cols:
        assert path["index_table"][img, c, 0, OBJECT] == 0


# ---- 3. a partial last block -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,D,inv", [(136, 48, None), (200, 32, 0.0)])
def test_partial_last_block(rows, D, inv, monkeypatch):
    """H % 64 != 0: in the first step of row H - 1 the lanes beyond vT hold the initial (+inf, -1) pairs."""
    ov = {} if inv is None else dict(invalid_disparity=inv)
    _check(helpers.build_case("drn_d_22_unary", rows, 96, D, seed=73, n_images=2, **ov), monkeypatch)


# ---- 4. the distrust path ----------------------------------------------------------------------------------------------
def test_distrusted_calls_repair_to_the_tile_path_bits(monkeypatch):
    case = helpers.build_case("drn_d_22_unary", 136, 64, 32, seed=79, n_images=2)
    tile, rep = _three_ways(case, monkeypatch, walk_modes=(("3", 1), ("3", 1)))
    assert np.array_equal(rep["cost_bits"], tile["cost_bits"])  # the repair writes every row
    assert np.array_equal(rep["index_table"], tile["index_table"])
