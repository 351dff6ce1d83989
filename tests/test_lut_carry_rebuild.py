"""The identity the unary walk (k_unary_path) builds the object data-cost table on, checked on the CPU: every entry of
the oracle's table, lutT[32 k + p + 1][fn], is output p of the reference's 32-lane Kogge-Stone network (shuffle
distances 1, 2, 4, 8, 16) over x_l = obj_cost_lut[fn][bin of row 32 k + l], whose lane 0 first adds the block's carry
lutT[32 k][fn] -- bit for bit, in float32.  Rows beyond the image use bin 0; a bin is (int)d clamped to [0, D - 1]."""
import numpy as np
import pytest

import helpers
from oracle import oracle


def _bins(dcol, H, nrows, D):
    d = np.zeros(nrows, np.float32)
    d[:H] = dcol
    return np.clip(d.astype(np.int32), 0, D - 1)


@pytest.mark.parametrize("preset,rows,cols,D,ov,hostile", [
    ("drn_d_22_unary", 200, 48, 48, {}, False),
    ("drn_d_22_unary", 136, 64, 64, dict(invalid_disparity=0.0), False),
    ("drn_d_22_unary", 256, 64, 128, {}, True),
    ("disparity_only_unary", 96, 32, 256, {}, False),
    ("drn_d_22_unary", 104, 64, 64, {}, True),
])
def test_lut_entries_rebuild_from_carry_rows(preset, rows, cols, D, ov, hostile):
    case = helpers.build_case(preset, rows, cols, D, seed=61, n_images=1, **ov)
    if hostile:      # zero, subnormal and D - 1.01 disparities, random ones
        case = helpers.make_hostile(case, seed=62)
    cfg, p = case["cfg"], case["params"]
    cost = np.ascontiguousarray(case["lut"], np.float32).reshape(D, D)              # [fn][dis]
    joined = oracle.join_columns(cfg, case["disparity"][0])
    H = rows
    nb = (H + 31) // 32
    for c in range(cfg.realcols):
        want = oracle.object_lut_column(p, joined[c], case["lut"])[:, : H + 1]      # [D][H + 1]
        dis = _bins(joined[c], H, 32 * nb, D)
        got = np.zeros_like(want)       # rebuilt from the carries of the oracle's own table, lanes = rows
        for k in range(nb):
            x = cost[:, dis[32 * k: 32 * k + 32]].copy()                            # [fn][lane]
            x[:, 0] = x[:, 0] + want[:, 32 * k]                                      # c[0] += carry
            for j in (1, 2, 4, 8, 16):
                prev = x.copy()
                x[:, j:] = prev[:, j:] + prev[:, :-j]                                # c[l] += c[l - j]
            n = min(32, H - 32 * k)
            got[:, 32 * k + 1: 32 * k + 1 + n] = x[:, :n]
        got[:, 0] = want[:, 0]
        assert np.array_equal(want[:, 0], np.zeros(D, np.float32))
        assert np.array_equal(helpers.bits(want), helpers.bits(got)), c
