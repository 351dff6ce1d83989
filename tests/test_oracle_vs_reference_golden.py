"""The CPU oracle against outputs recorded from the upstream reference's own code (hipified, built for
gfx950, run on an MI355X: tests/golden/make_reference_golden.py).  Bit for bit: the host precompute
(vhor), the column join, the object-LUT rows 0..H, the Sections up to each column's terminator, and
the instance candidates per class as a multiset (the reference appends them in atomic arrival
order).  No GPU and no reference needed: this holds the pin wherever the suite runs."""
import glob
import json
import os

import numpy as np
import pytest

import helpers
from instance_stixels_amd import make_config
from oracle import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_REF = sorted(glob.glob(os.path.join(HERE, "golden", "reference_hip", "*.npz")))


def test_fixtures_present():
    assert len(GOLDEN_REF) >= 12


def _candidates(out):
    recs = []
    for cls in range(8):
        m = int(out["inst_per_class"][cls])
        com = np.ascontiguousarray(out["inst_centerofmass"][cls][:m], np.float32).view(np.uint32)
        idx = out["inst_indices"][cls][:m]
        core = out["inst_core"][cls][:m] != 0
        recs += [(cls, int(idx[k, 0]), int(idx[k, 1]), int(com[k, 0]), int(com[k, 1]), int(core[k]))
                 for k in range(m)]
    return sorted(recs)


@pytest.mark.parametrize("path", GOLDEN_REF, ids=[os.path.basename(p)[:-4] for p in GOLDEN_REF])
def test_oracle_matches_the_reference_recording(path):
    g = np.load(path)
    spec = json.loads(str(g["case"]))
    cfg = make_config(spec["preset"], spec["rows"], spec["cols"], spec["max_dis"], **spec["overrides"])
    rows, C = int(cfg.rows), cfg.realcols
    params, lut, odr = oracle.host_initialize(cfg)
    vhor_image, tilt, height, alpha = g["road"]
    gf, ng, ig, vhor = oracle.host_ground(cfg, int(vhor_image), np.float32(tilt), np.float32(height),
                                          np.float32(alpha))
    assert vhor == int(g["vhor"])

    joined = oracle.join_columns(cfg, g["disparity"])
    assert np.array_equal(helpers.bits(joined), helpers.bits(g["joined"]))

    for c in range(C):
        want = oracle.object_lut_column(params, joined[c], lut)[:, : rows + 1]
        assert np.array_equal(helpers.bits(want), helpers.bits(g["object_lut"][c])), f"object LUT column {c}"

    out = oracle.compute(params, lut, odr, joined, g["segmentation"], gf, ng, ig, vhor, bool(cfg.pairwise),
                         want_tables=False)
    for c in range(C):
        n = helpers.n_sections(out["sections"][c])
        want = g["sections"][c]
        n_ref = int(np.argmax(want[:, 0] == -1))
        assert n == n_ref, f"column {c}: {n} sections in the oracle, {n_ref} in the reference"
        got = out["sections"][c][:n].view(np.int32).reshape(-1, 8)
        assert np.array_equal(got, want[:n]), f"column {c}: Sections differ"

    assert np.array_equal(out["inst_per_class"], g["inst_per_class"])
    want = sorted(tuple(int(v) for v in r) for r in g["candidates"])
    assert _candidates(out) == want
