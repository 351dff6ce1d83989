"""CPU checks of the parameter sweep (is_compute_sweep / is_recluster, Stixels::SweepBatch ...): the symbols are
declared, exported and bound; is_sweep_set as a C++ compiler lays it out against core.SweepSet; and the SweepSet ->
is_sweep_set weight rule against SetWeightParameters + GetParameters (PrecomputeHost needs no device)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from instance_stixels_amd import core, evaluation, host, make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "instance_stixels_core.h")).read()
    for name in ("is_compute_sweep", "is_recluster"):
        assert name + "(" in header, name
        assert hasattr(core.lib(), name) and name in core.EXPORTS, name
    for name in ("ish_sweep_batch", "ish_select_sweep_set", "ish_sweep_sections", "ish_recluster_batch",
                 "ish_core_sweep_set", "ish_last_frames", "ish_sweep_sets", "ish_active_device"):
        assert hasattr(host.lib(), name) and name in host.EXPORTS, name
    for name in ("SweepBatch", "SelectSweepSet", "SweepSections", "ReclusterBatch"):
        assert callable(getattr(host.Stixels, name)), name
    assert callable(core.Core.run_sweep) and callable(evaluation.sweep_scores)
    hpp = open(os.path.join(ROOT, "include", "InstanceStixels", "Stixels.hpp")).read()
    for name in ("struct SweepSet", "void SweepBatch(", "void SelectSweepSet(", "void SweepSections(",
                 "void ReclusterBatch("):
        assert name in hpp, name


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "instance_stixels_core.h"
#define F(f) printf(#f " %zu %zu\n", offsetof(is_sweep_set, f), sizeof(((is_sweep_set*)0)->f));
int main() {
    printf(". %zu 0\n", sizeof(is_sweep_set));
    FIELDS
    return 0;
}
"""


def test_sweep_set_size_and_offsets(tmp_path):
    src = PROBE.replace("FIELDS", "".join(f"F({n})" for n, _ in core.SweepSet._fields_))
    (tmp_path / "probe.cpp").write_text(src)
    exe = str(tmp_path / "probe")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "probe.cpp"), "-o", exe],
                   check=True)
    lines = [l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    got = {f: (int(off), int(size)) for f, off, size in lines}
    assert got["."][0] == 32 == ctypes.sizeof(core.SweepSet)
    assert len(got) == len(core.SweepSet._fields_) + 1
    for i, (name, _) in enumerate(core.SweepSet._fields_):
        field = getattr(core.SweepSet, name)
        assert got[name] == (field.offset, field.size) == (4 * i, 4), name
    assert [n for n, _ in core.SweepSet._fields_] == [
        "prior_weight", "disparity_weight", "segmentation_weight", "instance_weight", "clustering_eps",
        "clustering_min_pts", "clustering_size_filter", "reserved"]


# (prior, disparity, segmentation, instance): both sides of both thresholds of SetWeightParameters
WEIGHTS = [
    (1e4, 0.006993, 11.241965, 0.001731),
    (1.0, 0.0001, 4.7095, 0.003131),
    (1.0, 0.003, 0.47095, 0.003131),
    (1.0, 1.0, 0.0, 0.5),          # no segmentation: the instance weight is forced to 0
    (1.0, 1.0, 1e-5, 0.5),         # not above 1e-5 (the comparison is made in double)
    (1.0, 1.0, 1.1e-5, 0.5),
    (1.0, 1.0, 2.0, 0.9e-8),       # an instance weight below 1e-8 is 0
    (1.0, 1.0, 2.0, 1.1e-8),
    (2.5, 30.0, 3.0, 0.25),        # the rule does not look at the other weights
]


@pytest.mark.parametrize("w", WEIGHTS)
def test_weight_rule_is_set_weight_parameters(w):
    """Stixels::CoreSweepSet gives, bit for bit, the four weights GetParameters() shows after SetConfig (which calls
    SetWeightParameters) + PrecomputeHost with the same user-facing weights."""
    pw, dw, sw, iw = w
    cfg = make_config("drn_d_22_unary", 128, 256, 32, prior_weight=pw, disparity_weight=dw, segmentation_weight=sw,
                      instance_weight=iw, eps=7.5, min_pts=5, size_filter=11)
    st = host.Stixels()
    st.SetConfig(cfg)
    st.PrecomputeHost()
    p = st.GetParameters()
    s = host.core_sweep_set(pw, dw, sw, iw, 7.5, 5, 11)
    want = np.array([p.prior_weight, p.disparity_weight, p.segmentation_weight, p.instance_weight], np.float32)
    got = np.array([s.prior_weight, s.disparity_weight, s.segmentation_weight, s.instance_weight], np.float32)
    assert np.array_equal(want.view(np.uint32), got.view(np.uint32)), (want, got)
    assert np.float32(s.clustering_eps) == np.float32(7.5)
    assert (s.clustering_min_pts, s.clustering_size_filter, s.reserved) == (5, 11, 0)
    st.close()
