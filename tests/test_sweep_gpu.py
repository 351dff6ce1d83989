"""GPU tests of the parameter sweep: is_compute_sweep / is_recluster and Stixels::SweepBatch, SelectSweepSet,
SweepSections, ReclusterBatch.

One resident batch (128x256x32, two frames) is scored for three or four parameter sets in one call.  The yardstick is
always a FRESH host.Stixels / Core created with that set's parameters, never the sweep itself: every set's Sections
(up to each column's terminator, helpers.sections_equal) and instance outputs must carry the fresh object's bytes."""
import numpy as np
import pytest

import helpers
from instance_stixels_amd import core as core_mod
from instance_stixels_amd import host, make_config
from oracle import oracle

pytestmark = pytest.mark.gpu

ROWS, COLS, MAX_DIS = 128, 256, 32
PRESETS = ("drn_d_22_unary", "drn_d_38_pairwise")
WEIGHT_FIELDS = ("prior_weight", "disparity_weight", "segmentation_weight", "instance_weight")
SET_FIELDS = WEIGHT_FIELDS + ("eps", "min_pts", "size_filter")
_CACHE = {}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _case(preset, hostile=False):
    key = ("case", preset, hostile)
    if key not in _CACHE:
        case = helpers.build_case(preset, ROWS, COLS, MAX_DIS, seed=3, n_images=2)
        _CACHE[key] = helpers.make_hostile(case, 11) if hostile else case
    return _CACHE[key]


def _overrides(cfg):
    """The four sets of the issue: the preset's own, sw x 0.1, dw x 30, sw = 0 (instance weight forced to 0)."""
    return [{}, dict(segmentation_weight=cfg.segmentation_weight * 0.1),
            dict(disparity_weight=cfg.disparity_weight * 30), dict(segmentation_weight=0.0)]


def _cfg(preset, ov):
    return make_config(preset, ROWS, COLS, MAX_DIS, **ov)


def _host_set(cfg):
    return tuple(getattr(cfg, f) for f in SET_FIELDS)


def _road(case, n):
    return [(f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground) for f in case["frames"][:n]]


def _fresh_host(preset, ov, case, n=2, max_batch=2, with_instances=True, keep=False):
    """ComputeBatch of a fresh host.Stixels configured with the set's parameters: (data, maps[, the object])."""
    key = ("host", preset, tuple(sorted(ov.items())), id(case), n, max_batch, with_instances)
    if keep or key not in _CACHE:
        st = host.Stixels()
        st.SetConfig(_cfg(preset, ov))
        st.Initialize(max_batch=max_batch)
        big, seg = _dev(case["disparity"][:n]), _dev(case["segmentation"][:n])
        res = st.ComputeBatch(case["cfg"].pairwise, big.data_ptr(), seg.data_ptr(), _road(case, n),
                              with_instances=with_instances)
        if keep:
            return res + (st,)
        st.close()
        _CACHE[key] = res
    return _CACHE[key]


def _core_case(case, preset, ov):
    """The case with the parameter block of the set (the object tables do not depend on the seven parameters)."""
    cfg = _cfg(preset, ov)
    params, lut, odr = oracle.host_initialize(cfg)
    assert np.array_equal(lut, case["lut"]) and np.array_equal(odr, case["odr"])
    out = dict(case)
    out["cfg"], out["params"] = cfg, params
    return out


def _new_core(case, monkeypatch=None, env=None, max_batch=None):
    env = env or {}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return core_mod.Core(case["params"], case["lut"], case["odr"], max_batch=max_batch or len(case["frames"]))
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _run_kw(case):
    cfg = case["cfg"]
    return dict(disparity_big=case["disparity"], segmentation=case["segmentation"], ground_function=case["gf"],
                normalization_ground=case["ng"], inv_sigma2_ground=case["ig"], vhor=case["vhor"],
                pairwise=bool(cfg.pairwise), median_join=bool(cfg.median_join))


def _core_set(params, **changes):
    s = core_mod.SweepSet(params.prior_weight, params.disparity_weight, params.segmentation_weight,
                          params.instance_weight, params.clustering_eps, params.clustering_min_pts,
                          params.clustering_size_filter, 0)
    for k, v in changes.items():
        setattr(s, k, v)
    return s


INST = ("inst_centerofmass", "inst_indices", "inst_core", "inst_per_class", "inst_labels")


def _assert_core_equal(sweep, k, fresh, what):
    for img in range(len(fresh["sections"])):
        assert helpers.sections_equal(fresh["sections"][img], sweep["sections"][k][img]), \
            f"{what}: set {k} image {img}: Sections differ from the fresh context's"
    for name in INST:
        a, b = np.ascontiguousarray(fresh[name]), np.ascontiguousarray(sweep[name][k])
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}: set {k}: {name} differs"


def _core_sweep_against_fresh(case, preset, ovs, monkeypatch=None, env=None, what="", cases=None):
    """One sweep on a context of the first set against one fresh context per set, all created under `env`."""
    cases = cases or [_core_case(case, preset, ov) for ov in ovs]
    sets = [_core_set(c["params"]) for c in cases]
    c = _new_core(cases[0], monkeypatch, env)
    try:
        sweep = c.run_sweep(sets, **_run_kw(cases[0]))
    finally:
        c.close()
    for k, ck in enumerate(cases):
        f = _new_core(ck, monkeypatch, env)
        try:
            fresh = f.run(want_tables=False, **_run_kw(ck))
        finally:
            f.close()
        _assert_core_equal(sweep, k, fresh, what)
    return sweep


# ---- 1. both presets, the four sets --------------------------------------------------------------------------
@pytest.mark.parametrize("preset", PRESETS)
def test_every_set_equals_a_fresh_object(preset):
    case = _case(preset)
    ovs = _overrides(case["cfg"])
    # the condition: on this case at least three of the four sets give pairwise different Sections (CPU oracle)
    ref = []
    for ov in ovs:
        ck = _core_case(case, preset, ov)
        ref.append([helpers.run_oracle(ck, i)["sections"] for i in range(2)])
    different = lambda a, b: not all(helpers.sections_equal(ref[a][i], ref[b][i]) for i in range(2))  # noqa: E731
    assert any(all(different(a, b) for a in trio for b in trio if a < b)
               for trio in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3))), "the sets do not change the result"
    # the C ABI: Sections, candidates and labels of every set
    _core_sweep_against_fresh(case, preset, ovs, what=preset)
    # the host class: Sections and mappings of every set through SweepSections
    st = host.Stixels()
    st.SetConfig(case["cfg"])
    st.Initialize(max_batch=2)
    big, seg = _dev(case["disparity"]), _dev(case["segmentation"])
    st.SweepBatch(case["cfg"].pairwise, big.data_ptr(), seg.data_ptr(), _road(case, 2),
                  [_host_set(_cfg(preset, ov)) for ov in ovs])
    for k, ov in enumerate(ovs):
        data, maps = st.SweepSections(k)
        fdata, fmaps = _fresh_host(preset, ov, case)
        for i in range(2):
            assert helpers.sections_equal(fdata[i].sections, data[i].sections), (preset, k, i)
            assert data[i].vhor == fdata[i].vhor and data[i].alpha_ground == fdata[i].alpha_ground
            assert maps[i] == fmaps[i], (preset, k, i)
    st.close()


# ---- 2. the unary launch paths ---------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{"IS_UNARY_PATH": "0"}, {"IS_UNARY_PATH": "1"}, {"IS_UNARY_PATH": "3"},
                                 {"IS_NO_PRUNE": "1"}], ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()))
def test_unary_launch_paths(monkeypatch, env):
    preset = PRESETS[0]
    case = _case(preset)
    _core_sweep_against_fresh(case, preset, _overrides(case["cfg"]), monkeypatch, env, what=str(env))


def test_sets_that_disagree_on_the_walk(monkeypatch):
    """IS_UNARY_PATH=1 makes every pruned set walk at this size; a negative disparity weight switches the pruning of
    one set off (the weights_ok rule), which sends it down the tile path: the sweep prepares both tables."""
    preset = PRESETS[0]
    case = _case(preset)
    env = {"IS_UNARY_PATH": "1"}
    ovs = _overrides(case["cfg"])[:3]
    cases = [_core_case(case, preset, ov) for ov in ovs]
    cases[1] = dict(cases[1])
    p = core_mod.StixelParams.from_buffer_copy(cases[1]["params"])
    p.disparity_weight = -abs(p.disparity_weight)
    cases[1]["params"] = p
    _core_sweep_against_fresh(case, preset, ovs, monkeypatch, env, what="mixed", cases=cases)
    # (and the first context of such a sweep did walk, the fresh context of the negative set did not)
    for ck, want in ((cases[0], 1), (cases[1], 0)):
        c = _new_core(ck, monkeypatch, env)
        c.run(want_tables=False, **_run_kw(ck))
        assert c.unary_path()[0] == want
        c.close()


# ---- 3. generic columns ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", PRESETS)
def test_generic_columns_are_counted_for_every_set(monkeypatch, preset):
    """Hostile columns take the generic encoding; the launches that compute them leave at once when the generic-column
    counter is zero, so sets 1 and 2 differ from fresh contexts if set 0 consumed the count."""
    case = _case(preset, hostile=True)
    ovs = _overrides(case["cfg"])[:3]
    _core_sweep_against_fresh(case, preset, ovs, what="hostile " + preset)
    if not case["cfg"].pairwise:  # ... and with the walk in front of the generic launches
        _core_sweep_against_fresh(case, preset, ovs, monkeypatch, {"IS_UNARY_PATH": "1"}, what="hostile walk")
    else:  # ... and with phase 2 of large batches, whose generic-column launch is the one that reads the counter
        _core_sweep_against_fresh(case, preset, ovs, monkeypatch, {"IS_P2_SPLIT": "0"}, what="hostile two-column")


# ---- 4. state ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", PRESETS)
def test_a_sweep_leaves_the_object_as_it_was(preset):
    case = _case(preset)
    cfg = case["cfg"]
    ovs = _overrides(cfg)[:3]
    sets = [_host_set(_cfg(preset, ov)) for ov in ovs]
    big, seg = _dev(case["disparity"]), _dev(case["segmentation"])
    st = host.Stixels()
    st.SetConfig(cfg)
    st.Initialize(max_batch=2)
    before, maps_before = st.ComputeBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), _road(case, 2))
    params_before = bytes(st.GetParameters())
    # n_images == max_batch and n_images < max_batch: the two staging-copy paths
    for n in (2, 1):
        st.SweepBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), _road(case, n), sets)
        assert st.LastFrames() == n
        for k, ov in enumerate(ovs):
            data, maps = st.SweepSections(k)
            fdata, fmaps = _fresh_host(preset, ov, case)   # (frame 0 of the two-frame batch is the one-frame batch)
            for i in range(n):
                assert helpers.sections_equal(fdata[i].sections, data[i].sections), (n, k, i)
                assert maps[i] == fmaps[i], (n, k, i)
    assert bytes(st.GetParameters()) == params_before
    after, maps_after = st.ComputeBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), _road(case, 2))
    for i in range(2):
        assert helpers.sections_equal(before[i].sections, after[i].sections)
        assert maps_before[i] == maps_after[i]
    st.close()


def _assert_batch_is_fresh(st, preset, case, n, what):
    """A plain ComputeBatch of n frames on `st`, and a consumer behind it, against a fresh object's."""
    cfg = case["cfg"]
    big, seg = _dev(case["disparity"][:n]), _dev(case["segmentation"][:n])
    data, maps = st.ComputeBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), _road(case, n))
    assert st.SweepSets() == 0
    fdata, fmaps, fresh = _fresh_host(preset, {}, case, n=n, keep=True)
    for i in range(n):
        assert helpers.sections_equal(fdata[i].sections, data[i].sections), (what, i)
        assert maps[i] == fmaps[i], (what, i)
    assert sum(len(m) for m in fmaps) > 0, "the case has no instance candidates: nothing is compared"
    assert _objects_equal(st.InstanceObjectsBatch(n), fresh.InstanceObjectsBatch(n)), what
    assert st.GetInstanceStixels() == fresh.GetInstanceStixels(), what
    fresh.close()


@pytest.mark.parametrize("sweep", ["2 frames with instances", "1 set x 1 frame", "without instances"])
def test_compute_batch_after_a_sweep_writes_the_objects_own_arrays(sweep):
    """The first ComputeBatch after a sweep on an object that has computed NOTHING before: its instance arrays do not
    hold the answer already, so a call that wrote its candidates and labels into the sweep's arrays returns other
    mappings than a fresh object.  Also with more frames than the sweep had, and after a sweep without instances
    (whose instance block was never allocated)."""
    preset = PRESETS[0]
    case = _case(preset)
    cfg = case["cfg"]
    ovs = _overrides(cfg)[1:3]   # (not the object's own parameters: the sweep's arrays hold other results)
    big, seg = _dev(case["disparity"]), _dev(case["segmentation"])
    st = host.Stixels()
    st.SetConfig(cfg)
    st.Initialize(max_batch=2)
    if sweep == "1 set x 1 frame":
        st.SweepBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), _road(case, 1), [_host_set(_cfg(preset, ovs[0]))])
    else:
        st.SweepBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), _road(case, 2),
                      [_host_set(_cfg(preset, ov)) for ov in ovs], with_instances=sweep != "without instances")
        st.SelectSweepSet(1)
    _assert_batch_is_fresh(st, preset, case, 2, sweep)
    # ... and a Compute() behind another sweep
    st.SweepBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), _road(case, 1), [_host_set(_cfg(preset, ovs[0]))])
    f = case["frames"][1]
    st.SetDisparityImage(f.disparity)
    st.SetSegmentation(f.segmentation)
    st.SetRoadParameters(*_road(case, 2)[1])
    data = st.Compute(cfg.pairwise)
    fdata, fmaps = _fresh_host(preset, {}, case)
    assert helpers.sections_equal(fdata[1].sections, data.sections)
    assert st.GetInstanceStixels() == fmaps[1]
    st.close()


def test_a_sweep_without_instances(monkeypatch):
    """No instance outputs: a unary set that walks writes its Sections itself and the back-trace runs gated
    (CallPlan::walk_sections), per set.  IS_UNARY_PATH=1 selects the walk at this size, =3 makes every walk distrust
    itself."""
    preset = PRESETS[0]
    case = _case(preset)
    cfg = case["cfg"]
    ovs = _overrides(cfg)
    for hostile in (False, True):   # (hostile: generic columns, which the gated back-trace still takes)
        base = _case(preset, hostile=hostile)
        cases = [_core_case(base, preset, ov) for ov in ovs]
        for env in ({"IS_UNARY_PATH": "1"}, {"IS_UNARY_PATH": "3"}):
            c = _new_core(cases[0], monkeypatch, env)
            sweep = c.run_sweep([_core_set(ck["params"]) for ck in cases], want_instances=False, **_run_kw(cases[0]))
            assert c.unary_path()[0] == 1
            c.close()
            for k, ck in enumerate(cases):
                f = _new_core(ck, monkeypatch, env)
                fresh = f.run(want_tables=False, want_instances=False, **_run_kw(ck))
                f.close()
                for img in range(2):
                    assert helpers.sections_equal(fresh["sections"][img], sweep["sections"][k][img]), \
                        (hostile, env, k, img)
    # the host class
    big, seg = _dev(case["disparity"]), _dev(case["segmentation"])
    st = host.Stixels()
    st.SetConfig(cfg)
    st.Initialize(max_batch=2)
    st.SweepBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), _road(case, 2),
                  [_host_set(_cfg(preset, ov)) for ov in ovs], with_instances=False)
    for k, ov in enumerate(ovs):
        data, maps = st.SweepSections(k, with_instances=False)
        assert maps is None
        fdata = _fresh_host(preset, ov, case)[0]
        assert all(helpers.sections_equal(fdata[i].sections, data[i].sections) for i in range(2)), k
    with pytest.raises(ValueError, match="with instances"):
        st.SweepSections(0)
    with pytest.raises(ValueError, match="needs a compute call with instances"):
        st.ReclusterBatch(1.0, 1, 1)
    st.close()


# ---- 5. clustering-only sets --------------------------------------------------------------------------------------
CLUSTER_B = dict(eps=0.5, min_pts=1, size_filter=1)   # every candidate is large and a cluster of its own


def test_clustering_only_sets():
    preset = PRESETS[0]
    case = _case(preset)
    cfg = case["cfg"]
    ovs = [{}, CLUSTER_B]
    big, seg = _dev(case["disparity"]), _dev(case["segmentation"])
    st = host.Stixels()
    st.SetConfig(cfg)
    st.Initialize(max_batch=2)
    st.SweepBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), _road(case, 2), [_host_set(_cfg(preset, ov)) for ov in ovs])
    (d0, m0), (d1, m1) = st.SweepSections(0), st.SweepSections(1)
    for i in range(2):
        assert helpers.sections_equal(d0[i].sections, d1[i].sections)
    assert any(m0[i] != m1[i] for i in range(2)), "the clustering parameters do not change the mapping on this case"
    for k, (ov, maps) in enumerate(zip(ovs, (m0, m1))):
        fmaps = _fresh_host(preset, ov, case)[1]
        assert all(maps[i] == fmaps[i] for i in range(2)), k
    # ReclusterBatch on the selected set of a sweep: set 0 clustered with the parameters of set 1 is set 1
    st.SelectSweepSet(0)
    again = st.ReclusterBatch(CLUSTER_B["eps"], CLUSTER_B["min_pts"], CLUSTER_B["size_filter"])
    assert all(again[i] == m1[i] for i in range(2))
    assert all(st.SweepSections(0)[1][i] == m1[i] for i in range(2)) and st.SweepSections(1)[1] == m1
    st.close()


# ---- 6. ReclusterBatch -----------------------------------------------------------------------------------------------
def _objects_equal(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
               for x, y in zip(a, b))


def test_recluster_batch():
    preset = PRESETS[0]
    case = _case(preset)
    cfg = case["cfg"]
    big, seg = _dev(case["disparity"]), _dev(case["segmentation"])
    fdata, fmaps, fresh = _fresh_host(preset, CLUSTER_B, case, keep=True)
    fresh_objects = fresh.InstanceObjectsBatch(2)
    fresh.close()
    st = host.Stixels()
    st.SetConfig(cfg)
    st.Initialize(max_batch=2)
    data, maps = st.ComputeBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), _road(case, 2), with_instances=True)
    assert any(maps[i] != fmaps[i] for i in range(2))
    sections_before = _sections_of(st, 2)
    got = st.ReclusterBatch(CLUSTER_B["eps"], CLUSTER_B["min_pts"], CLUSTER_B["size_filter"])
    assert all(got[i] == fmaps[i] for i in range(2))
    assert np.array_equal(sections_before, _sections_of(st, 2)), "ReclusterBatch touched the Sections"
    assert _objects_equal(st.InstanceObjectsBatch(2), fresh_objects)
    # ... and back: the object's own parameters give the mapping of its ComputeBatch again
    back = st.ReclusterBatch(cfg.eps, cfg.min_pts, cfg.size_filter)
    assert all(back[i] == maps[i] for i in range(2))
    st.ComputeBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), _road(case, 2), with_instances=False)
    with pytest.raises(ValueError, match="needs a compute call with instances"):
        st.ReclusterBatch(1.0, 1, 1)
    st.close()


def _sections_of(st, n):
    """The Sections the consumers read, as bytes: every field of the world records but the instance id."""
    _, rec = st.WorldBatch(n)
    return np.concatenate([np.ascontiguousarray(rec[f]).view(np.uint8).reshape(-1)
                           for f in rec.dtype.names if f != "instance_id"])


# ---- 7. the consumers ----------------------------------------------------------------------------------------------
def test_consumers_read_the_selected_set():
    preset = PRESETS[1]
    case = _case(preset)
    cfg = case["cfg"]
    ovs = _overrides(cfg)[:3]
    big, seg = _dev(case["disparity"]), _dev(case["segmentation"])
    st = host.Stixels()
    st.SetConfig(cfg)
    st.Initialize(max_batch=2)
    # refused before anything is queued: too many frames, no sets
    with pytest.raises(ValueError, match="n_images outside"):
        st.SweepBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), _road(case, 2) + _road(case, 1),
                      [_host_set(cfg)])
    with pytest.raises(ValueError, match="no parameter sets"):
        st.SweepBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), _road(case, 2), [])
    with pytest.raises(ValueError, match="not a SweepBatch"):
        st.SelectSweepSet(0)
    st.SweepBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), _road(case, 2), [_host_set(_cfg(preset, ov)) for ov in ovs])
    for k in (0, 2, 1):
        if k:   # (set 0 is selected by SweepBatch itself)
            st.SelectSweepSet(k)
        _, _, fresh = _fresh_host(preset, ovs[k], case, keep=True)
        assert np.array_equal(st.RenderBatch(2)[2], fresh.RenderBatch(2)[2]), k
        assert _objects_equal(st.InstanceObjectsBatch(2), fresh.InstanceObjectsBatch(2)), k
        (off, rec), (foff, frec) = st.WorldBatch(2), fresh.WorldBatch(2)
        assert np.array_equal(off, foff) and np.array_equal(rec.view(np.uint8), frec.view(np.uint8)), k
        fresh.close()
    with pytest.raises(ValueError, match="outside the sets"):
        st.SelectSweepSet(len(ovs))
    with pytest.raises(ValueError, match="outside the sets"):
        st.SelectSweepSet(-1)
    st.ComputeBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), _road(case, 2))
    with pytest.raises(ValueError, match="not a SweepBatch"):
        st.SelectSweepSet(0)
    st.close()


def test_sweep_scores_walks_the_sets():
    from instance_stixels_amd import evaluation
    preset = PRESETS[0]
    case = _case(preset)
    cfg = case["cfg"]
    ovs = _overrides(cfg)[:3]
    big, seg = _dev(case["disparity"]), _dev(case["segmentation"])
    rng = np.random.default_rng(5)
    gt_label = _dev(rng.integers(0, 34, (2, cfg.rows, cfg.cols)).astype(np.uint8))
    gt_inst = _dev((rng.integers(0, 3, (2, cfg.rows, cfg.cols)) * 26001).astype(np.int32))
    st = host.Stixels()
    st.SetConfig(cfg)
    st.Initialize(max_batch=2)
    st.SweepBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), _road(case, 2), [_host_set(_cfg(preset, ov)) for ov in ovs])
    sets = [_host_set(_cfg(preset, ov)) for ov in ovs]
    assert st.SweepSets() == len(sets) and st.GetActiveDevice() == 0
    with pytest.raises(ValueError, match="2 sets given"):
        evaluation.sweep_scores(st, sets[:2], gt_label.data_ptr(), gt_inst.data_ptr())
    scores = evaluation.sweep_scores(st, sets, gt_label.data_ptr(), gt_inst.data_ptr())
    st.close()
    import torch
    for k, ov in enumerate(ovs):
        _, _, fresh = _fresh_host(preset, ov, case, keep=True)
        conf = torch.zeros((34, 34), dtype=torch.int64, device="cuda")
        count = fresh.RenderBatch(2, gt_label=gt_label.data_ptr(), confusion=conf.data_ptr())[2]
        tables = fresh.InstanceOverlapBatch(2, gt_inst.data_ptr())
        fresh.close()
        assert np.array_equal(scores[k]["confusion"], conf.cpu().numpy().astype(np.uint64)), k
        assert np.array_equal(scores[k]["stixel_count"], count), k
        assert all(np.array_equal(a, b) for a, b in zip(scores[k]["overlaps"], tables)), k


# ---- 8. the C ABI directly -----------------------------------------------------------------------------------------
def test_c_abi_canaries_and_refusals():
    import torch
    preset = PRESETS[0]
    case = _case(preset)
    ovs = _overrides(case["cfg"])[:3]
    cases = [_core_case(case, preset, ov) for ov in ovs]
    sets = [_core_set(c["params"]) for c in cases]
    c = _new_core(cases[0])
    out = c.run_sweep(sets, canary=64, **_run_kw(cases[0]))
    for name in ("sections_guard", "labels_guard"):
        front, back, pattern = out[name]
        assert (front == pattern).all() and (back == pattern).all(), name + ": written outside the array"
    fresh = helpers.run_core(cases[2], want_tables=False)
    _assert_core_equal(out, 2, fresh, "canary run")
    # refusals: nothing is queued
    p = c.params
    n, C, S, H = 2, p.cols, p.max_sections, p.rows
    dev = torch.device("cuda", 0)
    joined = torch.zeros((n, C, H), dtype=torch.float32, device=dev)
    seg = _dev(case["segmentation"])
    sections = torch.zeros((len(sets), n, C, S, 8), dtype=torch.int32, device=dev)
    args = (joined.data_ptr(), seg.data_ptr(), case["gf"], case["ng"], case["ig"], case["vhor"], False, n)
    assert c.compute_sweep_ptr(*args, [], sections.data_ptr()) == -1           # n_sets < 1
    assert b"n_sets" in core_mod.lib().is_last_error()
    bad = _core_set(p)
    bad.reserved = 7
    assert c.compute_sweep_ptr(*args, [sets[0], bad], sections.data_ptr()) == -1
    assert b"reserved" in core_mod.lib().is_last_error()
    three = helpers.build_case(preset, ROWS, COLS, MAX_DIS, seed=3, n_images=3)
    assert c.compute_sweep_ptr(joined.data_ptr(), seg.data_ptr(), three["gf"], three["ng"], three["ig"], three["vhor"],
                               False, 3, sets, sections.data_ptr()) == -1     # n_images > max_batch
    assert b"n_images outside [1, max_batch]" in core_mod.lib().is_last_error()
    # is_recluster: every array of every image is required
    slots = C * S
    com = torch.zeros((8, slots, 2), dtype=torch.float32, device=dev)
    idx = torch.zeros((8, slots, 2), dtype=torch.int32, device=dev)
    cor = torch.zeros((8, slots), dtype=torch.uint8, device=dev)
    per = torch.zeros((8,), dtype=torch.int32, device=dev)
    lab = torch.zeros((8, slots), dtype=torch.int32, device=dev)
    full = core_mod.InstanceBuffers(com.data_ptr(), idx.data_ptr(), cor.data_ptr(), per.data_ptr(), lab.data_ptr(), None)
    no_idx = core_mod.InstanceBuffers(com.data_ptr(), None, cor.data_ptr(), per.data_ptr(), lab.data_ptr(), None)
    assert c.recluster_ptr(sections.data_ptr(), 1, 1.0, 1, 1, [no_idx]) == -1
    assert b"d_indices" in core_mod.lib().is_last_error()
    assert c.recluster_ptr(sections.data_ptr(), 1, 1.0, 1, 1, [full]) == 0
    torch.cuda.synchronize(dev)
    # ... and the context still computes what it computed
    again = c.run(want_tables=False, **_run_kw(cases[0]))
    _assert_core_equal(out, 0, again, "after the refusals")
    c.close()
