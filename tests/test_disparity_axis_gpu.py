"""The DP at every disparity count at which its code changes path.  is_ctx_create accepts any max_dis in [2, 1024]
whose LDS need stays under 160 KiB per workgroup; the kernels and plan_call branch on max_dis in more places than on
the rows, and the rest of the suite runs multiples of 8 up to 256 and one unary call at 320.

Shape: 136 rows (tiles of 64, 64 and 8 rows, H % 32 != 0), 64 image columns (8 stixel columns), seed = D; every call
requests tables.  Sections, cost table and index table must be bit-equal to the oracle (helpers.compare; the walk at
the rows it visits), through every unary route of test_unary_routes_gpu and every pairwise route of
test_pairwise_phase2_routes_gpu, the latter also with IS_P1_WIN_TILES = the number of tiles (it forces fn windows where
IS_P1_WINDOWED(D) allows them and must change nothing where it does not).  A route that a D cannot have (windows at
D % 4 != 0 or D <= 32, the fused LUT launch at three fn blocks or D > 256, the ring kernel above 256) must be left
silently and still give the oracle's bits.  The object table is compared directly as well: every entry of every column
on the windowed route, rows 32 k on the walk route (the DP sees the table only through minima of differences, and its
column D - 1 only where a mean reaches it).

    D                what it reaches
    2, 3, 5, 7       less than one quad per row; D = 2 divides the thread count without being a multiple of 4
    33, 34           above IS_P1_WIN with D % 4 = 1 and 2: not windowed although D > 32
    36               the smallest windowed D
    63, 65, 66       k_lut_carry<1> with dword staging; <2> with odd D (no pair stores); <2> with D % 4 = 2
    127, 129, 130    LutRow<2> -> gather, isf_nvr 2 -> 4, k_lut_carry -> k_prepare_fused<true>; three fn blocks
    193              four fn blocks with D % 4 = 1
    255, 257, 260    the last ring-kernel shapes, then none; 260 is windowed, 257 is not
    513              nine fn blocks, a phase-1 tile of 131 KiB
    D_max            the largest count is_ctx_create accepts at 136 rows, asked of the library

Inputs: helpers.ramp_columns puts a ramp 0.25 .. D - 0.25 into stixel column 0 and the constant D - 0.5 into column 1,
so that the first and the last disparity bin are reached by a mean and not through clamping; every case asserts that on
the oracle's joined disparity.  D in {33, 65, 130, 257} also run with invalid_disparity = 0, two images and a second
horizon; D in {34, 129, 260} also with helpers.make_hostile, generic columns beside FAST ones."""
import functools

import numpy as np
import pytest

import helpers
import test_pairwise_phase2_routes_gpu as pw
import test_unary_path_gpu as walk
import test_unary_routes_gpu as un
from instance_stixels_amd import make_config
from oracle import oracle

pytestmark = pytest.mark.gpu

ROWS, COLS = 136, 64
NTILES, QB = (ROWS + 63) // 64, 32
KNOBS = un.KNOBS + ("IS_P2_SPLIT", "IS_P2X", "IS_PW_GROUPS", "IS_NO_PRUNE")
TABLE = (2, 3, 5, 7, 33, 34, 36, 63, 65, 66, 127, 129, 130, 193, 255, 257, 260, 513)
CASES = ([(D, "plain") for D in TABLE] + [(D, "invalid-2img") for D in (33, 65, 130, 257)] +
         [(D, "hostile") for D in (34, 129, 260)])


def _case_id(c):
    return "D%d-%s" % c


def _build(preset, D, variant):
    """-> (case, the oracle's result per image); the input condition is asserted here, before any kernel runs."""
    n = 2 if variant == "invalid-2img" else 1
    ov = dict(invalid_disparity=0.0) if variant == "invalid-2img" else {}
    case = helpers.build_case(preset, ROWS, COLS, D, seed=D, n_images=n, **ov)
    assert case["cfg"].realcols == 8
    if n == 2:
        un._second_horizon(case, 39)
    if variant == "hostile":
        helpers.make_hostile(case, seed=7000 + D)
    helpers.ramp_columns(case)
    refs = [helpers.run_oracle(case, image=i) for i in range(n)]
    for r in refs:
        assert helpers.reaches_both_end_bins(r["joined"], D), "the inputs miss bin 0 or bin D - 1"
    return case, refs


def _check_unary(D, variant, monkeypatch):
    case, refs = _build(un.PRESET, D, variant)
    cfg, p, n = case["cfg"], case["params"], len(case["frames"])
    C = cfg.realcols
    # lutT[v][fn] of every column as the oracle builds it
    want_lut = [oracle.object_lut_column(p, refs[i]["joined"][c], case["lut"])[:, : ROWS + 1].T
                for i in range(n) for c in range(C)]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for name, env in un.ROUTES:
        table = carries = None
        core = walk._core(case, monkeypatch, env)
        try:
            got = walk._run(core, case, want_tables=True, prefill=True)
            state, carry_lds = core.unary_path(), core.lut_carry_lds()[0]
            if name == "windowed":
                table = [core.read_object_lut(c) for c in range(n * C)]
            if name == "walk":
                carries = [core.read_lut_carries(c) for c in range(n * C)]
        finally:
            core.close()
        # plan_call: unary_walk at IS_UNARY_PATH >= 2, distrusted at 3; lut_carry_lds = walk && the prepare launch
        # builds the table (no walk call fuses it) && isk_lut_carry_lds_bytes != 0, i.e. at most two fn blocks
        walks = name in ("walk", "distrusted-walk")
        expect = {"walk": (1, 0), "distrusted-walk": (1, 1)}.get(name)
        assert (state == expect) if expect else (state[0] == 0), (name, state)
        assert carry_lds == (1 if walks and D <= 128 else 0), (name, carry_lds)
        got["cost_table"] = got["cost_bits"].view(np.float32)
        for i in range(n):
            errs = helpers.compare(refs[i], got, i, cfg, check_tables=name != "walk")
            errs += (un._visited_rows_match(refs[i], got, i, cfg) if name == "walk"
                     else un._initial_indices_match(refs[i], got, i, cfg))
            assert not errs, name + ", image %d:\n" % i + "\n".join(errs[:10])
        if table is not None:
            for c in range(n * C):
                bad = helpers.bits(want_lut[c]) != helpers.bits(table[c])
                assert not bad.any(), "object table, column %d: %d entries differ, first (v, fn) %s" % (
                    c, int(bad.sum()), np.argwhere(bad)[:5].tolist())
        if carries is not None:
            nb = (ROWS + 31) // 32
            for c in range(n * C):
                bad = helpers.bits(want_lut[c][0: 32 * nb: 32]) != helpers.bits(carries[c])
                assert not bad.any(), "carry rows, column %d: %d entries differ, first (k, fn) %s" % (
                    c, int(bad.sum()), np.argwhere(bad)[:5].tolist())


def _check_pairwise(D, variant, monkeypatch):
    case, refs = _build(pw.PRESET, D, variant)
    cfg, n = case["cfg"], len(case["frames"])
    n_blk = (ROWS - 1 + QB - 1) // QB          # the bound blocks that hold a candidate row (as in the routes' test)
    first = None
    for win in (None, NTILES):
        for name, env in pw.ROUTES:
            for k in KNOBS:
                monkeypatch.delenv(k, raising=False)
            what = name + ("" if win is None else ", IS_P1_WIN_TILES=%d" % win)
            got, summ = pw._run_route(case, env if win is None else dict(env, IS_P1_WIN_TILES=str(win)), monkeypatch)
            for i in range(n):
                errs = helpers.compare(refs[i], got, i, cfg)
                assert not errs, what + ", image %d:\n" % i + "\n".join(errs[:10])
            sb = helpers.bits(summ[:, 1:n_blk + 1])
            if first is None:
                first = sb
            else:
                bad = np.argwhere(sb != first)
                assert bad.size == 0, "%s: %d summary words differ from the default route, first (column, block - 1, float): %s" % (
                    what, len(bad), bad[:8].tolist())
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("c", CASES, ids=_case_id)
def test_unary_routes_at_the_disparity_counts_where_the_code_changes_path(c, monkeypatch):
    _check_unary(c[0], c[1], monkeypatch)


@pytest.mark.parametrize("c", CASES, ids=_case_id)
def test_pairwise_routes_at_the_disparity_counts_where_the_code_changes_path(c, monkeypatch):
    _check_pairwise(c[0], c[1], monkeypatch)


# ---- the bound of the accepted range ------------------------------------------------------------------------------

def _create(params, lut, odr):
    from instance_stixels_amd.core import Core
    Core(params, lut, odr, max_batch=1).close()


@functools.lru_cache(maxsize=None)
def _bound():
    """(D_max, [(D, error text)] of the refused counts above it): max_dis = 640, 639, ... at 136 rows until
    is_ctx_create accepts one.  A refusal happens in ctx_init before any allocation."""
    from instance_stixels_amd.core import CoreError
    refused = []
    for D in range(640, 512, -1):
        cfg = make_config(un.PRESET, ROWS, COLS, D)
        try:
            _create(*oracle.host_initialize(cfg))
        except CoreError as e:
            refused.append((D, str(e)))
            continue
        return D, refused
    return None, refused


def test_the_accepted_range_ends_where_the_lds_bound_says():
    from instance_stixels_amd.core import CoreError, StixelParams
    D_max, refused = _bound()
    print("largest accepted max_dis at %d rows: %s (%d counts refused from 640 down)" % (ROWS, D_max, len(refused)))
    assert refused and refused[0][0] == 640, "64 * 641 * 4 bytes alone exceed 160 KiB"
    for D, text in refused:
        assert "more than 160 KiB of LDS" in text, (D, text)
    assert D_max is not None, "64 * 514 * 4 = 131 584 bytes leave 32 KiB for the rest: 513 must be accepted"
    params, _, _ = oracle.host_initialize(make_config(un.PRESET, ROWS, COLS, 32))
    for D in (1, 0, 1025):
        p = StixelParams.from_buffer_copy(params)
        p.max_dis = D
        with pytest.raises(CoreError, match="max_dis out of range"):
            _create(p, np.zeros((D, D), np.float32), np.zeros(D, np.float32))


def test_unary_routes_at_the_largest_accepted_disparity_count(monkeypatch):
    """Accepted means launchable and correct."""
    D_max = _bound()[0]
    assert D_max is not None
    _check_unary(D_max, "plain", monkeypatch)


def test_pairwise_routes_at_the_largest_accepted_disparity_count(monkeypatch):
    D_max = _bound()[0]
    assert D_max is not None
    _check_pairwise(D_max, "plain", monkeypatch)
