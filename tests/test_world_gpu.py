"""The stixel world on the MI355X: Stixels::WorldBatch / is_stixel_world (is_k_world.hip) against the host
composition on the same call's output -- the Sections of ComputeBatch field for field (floats bitwise), the
instance mapping per (column, section), and Get3DVertices' twelve floats per stixel.  Vertex rule: identical
bits, except that where the host value is NaN the device value must be NaN (the payload and sign of a NaN differ
between x86 and gfx950 and are not part of the contract); +-inf must match in sign."""
import numpy as np
import pytest

import helpers
import world_reference as wr
from instance_stixels_amd import core, host, synthetic, world
from instance_stixels_amd.config import SECTION_DTYPE

pytestmark = pytest.mark.gpu

# (rows, cols, max_dis, n, overrides): the shapes of tests/test_render_gpu.py (64x72: cols is not realcols * 8)
SHAPES = [(256, 512, 64, 4, {}), (1024, 2048, 128, 8, {}), (784, 1792, 128, 2, dict(invalid_disparity=0.0)),
          (64, 72, 32, 2, dict(width_margin=8))]
PRESETS = ["drn_d_22_unary", "drn_d_38_unary", "drn_d_22_pairwise", "drn_d_38_pairwise"]
GUARD = 0x5A5A5A5A


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _dev(a):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _setup(preset, rows, cols, D, n, ov, seed, with_instances=True):
    ov = dict(ov, size_filter=10 if preset.endswith("unary") else 8)
    case = helpers.build_case(preset, rows, cols, D, seed=seed, n_images=n, **ov)
    cfg = case["cfg"]
    frames = [synthetic.make_frame(cfg, seed=seed + 100 * i, n_slabs=10 + 2 * i, offset_scale=1.0)
              for i in range(n)]
    st = host.Stixels()
    st.SetConfig(cfg)
    st.Initialize(max_batch=n)
    big, seg = _dev(np.stack([f.disparity for f in frames])), _dev(np.stack([f.segmentation for f in frames]))
    # different road parameters per frame (the horizon and the slope move with the frame index)
    road = [(f.vhor_image + 3 * i, f.camera_tilt, f.camera_height, f.alpha_ground * (1.0 + 0.07 * i))
            for i, f in enumerate(frames)]
    data, maps = st.ComputeBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), road, with_instances=with_instances)
    return st, cfg, (big, seg, road), data, maps


def _host_composition(st, data, mapping):
    """The records of one frame as a caller composes them today: Sections + mapping lookups + Get3DVertices."""
    col, idx = wr.used(data.sections)
    sec = data.sections[col, idx]
    rec = np.zeros(len(sec), core.WORLD_DTYPE)
    rec["column"], rec["section"] = col, idx
    for name in SECTION_DTYPE.names:
        rec[name] = sec[name]
    rec["instance_id"] = [(mapping or {}).get((int(c), int(i)), -1) for c, i in zip(col, idx)]
    rec["vertices"] = st.Get3DVertices(data).reshape(-1, 12)
    return rec


def _check_batch(st, data, maps, offsets, records):
    n = len(offsets) - 1
    assert offsets[0] == 0 and offsets[-1] == len(records)
    for i in range(n):
        got = records[offsets[i]:offsets[i + 1]]
        want = _host_composition(st, data[i], maps[i] if maps else None)
        wr.assert_records_equal(got, want)
        inf = np.isinf(want["vertices"])
        assert np.array_equal(np.signbit(got["vertices"][inf]), np.signbit(want["vertices"][inf]))
    assert not records["reserved"].any()


@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("rows, cols, D, n, ov", SHAPES)
def test_world_batch_matches_host_composition(preset, rows, cols, D, n, ov):
    st, cfg, _, data, maps = _setup(preset, rows, cols, D, n, ov, seed=rows + n)
    offsets, records = st.WorldBatch(n)
    _check_batch(st, data, maps, offsets, records)
    if rows >= 256:
        assert (records["instance_id"] >= 0).any(), "no labelled stixel: the case does not exercise the ids"
    assert len({d.vhor for d in data}) > 1 and len({d.alpha_ground for d in data}) > 1
    st.close()


@pytest.mark.parametrize("preset", ["drn_d_22_unary", "drn_d_38_pairwise"])
def test_world_after_single_compute(preset):
    rows, cols, D = 256, 512, 64
    case = helpers.build_case(preset, rows, cols, D, seed=5, size_filter=10 if preset.endswith("unary") else 8)
    cfg = case["cfg"]
    f = synthetic.make_frame(cfg, seed=5, n_slabs=16, offset_scale=1.0)
    st = host.Stixels()
    st.SetConfig(cfg)
    st.Initialize()
    st.SetDisparityImage(f.disparity)
    st.SetSegmentation(f.segmentation)
    st.SetRoadParameters(f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground)
    data = st.Compute(cfg.pairwise)
    mapping = st.GetInstanceStixels()
    offsets, records = st.WorldBatch(1)
    _check_batch(st, [data], [mapping], offsets, records)
    assert (records["instance_id"] >= 0).any()
    st.close()


def test_world_without_instances_has_no_ids():
    st, cfg, _, data, maps = _setup("drn_d_22_unary", 256, 512, 64, 3, {}, seed=11, with_instances=False)
    assert maps is None
    offsets, records = st.WorldBatch(3)
    _check_batch(st, data, None, offsets, records)
    assert (records["instance_id"] == -1).all()
    st.close()


def _hand_built(rows=64, C=6, S=8, n=2):
    """Sections of n frames x C columns with every column end of the contract and the zero disparities."""
    rng = np.random.default_rng(4)
    secs = np.zeros((n, C, S), SECTION_DTYPE)
    secs["type"] = rng.integers(0, 3, secs.shape)
    secs["vB"] = rng.integers(0, rows, secs.shape)
    secs["vT"] = rng.integers(0, rows, secs.shape)
    secs["disparity"] = rng.uniform(0.5, 30, secs.shape)
    secs["semantic_class"] = rng.integers(0, 19, secs.shape)
    for name in ("cost", "instance_meanx", "instance_meany"):
        secs[name] = rng.normal(0, 100, secs.shape)
    for i in range(n):
        secs["type"][i, 0, 0] = -1                       # terminator in slot 0: no record
        secs["type"][i, 1, 3] = -1
        secs["type"][i, 3, 1] = -1
        secs["type"][i, 4, S - 1] = -1                   # full column with a terminator in the last slot
        secs["type"][i, 5, 5] = -1
    # column 2 keeps no terminator: max_sections - 1 records
    vhor = [20, 31]
    secs[0, 1, 0] = (1, 3, 9, 0.0, 13, 1.0, 2.0, 3.0)          # object at disparity 0
    secs[1, 3, 0] = (0, 4, vhor[1], 2.0, 0, 1.0, 0.0, 0.0)     # ground with vT == vhor
    secs[0, 5, 1] = (0, vhor[0], 40, 2.0, 1, 1.0, 0.0, 0.0)    # ground with vB == vhor
    inst = rng.integers(-1, 40, secs.shape).astype(np.int32)
    return secs, inst, vhor, [0.25, 0.125]


CAMERA = dict(focal=707.0, baseline=0.54, camera_center_x=21.5, camera_center_y=30.25)


def _run_abi(secs, inst, vhor, alpha, capacity, rows=64, step=8, guard=64):
    torch, dev = _torch()
    n, C, S = secs.shape
    d_sec = _dev(secs.view(np.int32).reshape(n, C, S, 8))
    d_inst = None if inst is None else _dev(inst)
    d_counts = torch.full((n * C,), -7, dtype=torch.int32, device=dev)
    d_offsets = torch.full((n * C + 1,), -7, dtype=torch.int32, device=dev)
    d_totals = torch.full((n,), -7, dtype=torch.int32, device=dev)
    d_world = torch.full(((capacity + guard) * 24,), GUARD, dtype=torch.int32, device=dev)
    core.stixel_world_ptr(alpha, vhor, d_sections=d_sec.data_ptr(),
                          d_section_instance=None if inst is None else d_inst.data_ptr(), n_images=n, realcols=C,
                          max_sections=S, rows=rows, column_step=step, capacity=capacity,
                          d_counts=d_counts.data_ptr(), d_offsets=d_offsets.data_ptr(),
                          d_frame_totals=d_totals.data_ptr(), d_world=d_world.data_ptr(), **CAMERA)
    torch.cuda.synchronize()
    w = d_world.cpu().numpy()
    return (d_counts.cpu().numpy(), d_offsets.cpu().numpy(), d_totals.cpu().numpy(),
            w[:capacity * 24].view(core.WORLD_DTYPE), w[capacity * 24:], d_sec)


def _want_abi(secs, inst, vhor, alpha, rows=64, step=8):
    out = []
    for i in range(secs.shape[0]):
        mapping = None
        if inst is not None:
            mapping = {(c, s): int(inst[i, c, s]) for c in range(secs.shape[1]) for s in range(secs.shape[2])}
        out.append(wr.records(secs[i], mapping, rows, step, CAMERA["focal"], CAMERA["baseline"],
                              CAMERA["camera_center_x"], CAMERA["camera_center_y"], alpha[i], vhor[i]))
    return out


@pytest.mark.parametrize("with_map", [True, False])
def test_c_abi_hand_built_sections(with_map):
    torch, dev = _torch()
    secs, inst, vhor, alpha = _hand_built()
    inst = inst if with_map else None
    n, C, S = secs.shape
    want = _want_abi(secs, inst, vhor, alpha)
    flat = np.concatenate(want)
    total = len(flat)
    per_col = [0, 3, S - 1, 1, S - 1, 5]
    assert [len(w) for w in want] == [sum(per_col)] * n
    counts, offsets, totals, world_rec, guard, d_sec = _run_abi(secs, inst, vhor, alpha, total)
    # counts / offsets identical to is_pack_sections on the same input
    p_counts = torch.zeros(n * C, dtype=torch.int32, device=dev)
    p_offsets = torch.zeros(n * C + 1, dtype=torch.int32, device=dev)
    p_packed = torch.zeros((n * C * S, 8), dtype=torch.int32, device=dev)
    core.pack_sections_ptr(d_sec.data_ptr(), n * C, S, p_counts.data_ptr(), p_offsets.data_ptr(), p_packed.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(counts, p_counts.cpu().numpy()) and np.array_equal(offsets, p_offsets.cpu().numpy())
    assert counts.tolist() == per_col * n and offsets[-1] == total and totals.tolist() == [len(w) for w in want]
    wr.assert_records_equal(world_rec, flat)
    assert np.isinf(flat["vertices"]).any(), "the zero disparities are not among the records"
    inf = np.isinf(flat["vertices"])
    assert np.array_equal(np.signbit(world_rec["vertices"][inf]), np.signbit(flat["vertices"][inf]))
    assert (guard == GUARD).all()
    if not with_map:
        assert (world_rec["instance_id"] == -1).all()
    # a capacity smaller than the total: the prefix, nothing at or beyond it, the true total in the offsets
    for cap in (total - 1, 10, 0):
        counts2, offsets2, totals2, rec2, guard2, _ = _run_abi(secs, inst, vhor, alpha, cap)
        assert (guard2 == GUARD).all(), f"capacity {cap}: a record was written behind the buffer"
        assert offsets2[-1] == total and np.array_equal(offsets2, offsets) and np.array_equal(totals2, totals)
        wr.assert_records_equal(rec2, flat[:cap])


def test_c_abi_long_columns_and_many_frames():
    """Columns of more than 64 sections (several rounds of the wave, a capacity that ends inside a round) and more
    frames than one launch takes (65 > 64), every frame with its own road parameters."""
    rows, C, S, n = 256, 3, 200, 65
    rng = np.random.default_rng(9)
    secs = np.zeros((n, C, S), SECTION_DTYPE)
    secs["type"] = rng.integers(0, 3, secs.shape)
    secs["vB"] = rng.integers(0, rows, secs.shape)
    secs["vT"] = rng.integers(0, rows, secs.shape)
    secs["disparity"] = rng.uniform(0.5, 60, secs.shape)
    secs["semantic_class"] = rng.integers(0, 19, secs.shape)
    for name in ("cost", "instance_meanx", "instance_meany"):
        secs[name] = rng.normal(0, 100, secs.shape)
    per_col = [150, 70, S - 1]              # three rounds, two rounds, no terminator: four rounds
    secs["type"][:, 0, 150] = -1
    secs["type"][:, 1, 70] = -1
    secs["type"][64, 1, 0] = -1             # the last frame (second launch): an empty column
    inst = rng.integers(-1, 900, secs.shape).astype(np.int32)
    vhor = [int(v) for v in rng.integers(100, 160, n)]
    alpha = [float(x) for x in rng.uniform(0.1, 0.4, n).astype(np.float32)]
    want = _want_abi(secs, inst, vhor, alpha, rows=rows)
    flat = np.concatenate(want)
    total = sum(per_col) * n - 70
    assert len(flat) == total and len(want[64]) == sum(per_col) - 70
    counts, offsets, totals, rec, guard, _ = _run_abi(secs, inst, vhor, alpha, total, rows=rows)
    assert counts.tolist() == per_col * 64 + [150, 0, S - 1] and offsets[-1] == total
    assert totals.tolist() == [len(w) for w in want] and (guard == GUARD).all()
    wr.assert_records_equal(rec, flat)
    assert np.array_equal(rec["section"][:150], np.arange(150))
    # capacities that end inside the second / third round of a column, in the first and in the second launch
    first = sum(per_col)
    for cap in (100, 64, 150 + 70 + 130, 64 * first + 129, 64 * first + 150 + 65):
        _, offsets2, totals2, rec2, guard2, _ = _run_abi(secs, inst, vhor, alpha, cap, rows=rows)
        assert (guard2 == GUARD).all(), f"capacity {cap}: a record was written behind the buffer"
        assert offsets2[-1] == total and np.array_equal(totals2, totals)
        wr.assert_records_equal(rec2, flat[:cap])


def test_host_class_paths():
    torch, dev = _torch()
    n = 4
    st, cfg, (big, seg, road), data, maps = _setup("drn_d_38_pairwise", 256, 512, 64, n, {}, seed=21)
    off_a, rec_a = st.WorldBatch(n)
    off_b, rec_b = st.WorldBatch(n)
    assert np.array_equal(off_a, off_b) and rec_a.tobytes() == rec_b.tobytes()
    _check_batch(st, data, maps, off_a, rec_a)
    # a subset equals the prefix
    off_2, rec_2 = st.WorldBatch(2)
    assert np.array_equal(off_2, off_a[:3]) and rec_2.tobytes() == rec_a[:off_a[2]].tobytes()
    # a tiny capacity forces the repeat with the true total; a roomy one does not: identical results
    st.SetWorldCapacity(1)
    off_t, rec_t = st.WorldBatch(n)
    st.SetWorldCapacity(st.GetRealCols() * (st.GetMaxSections() - 1))
    off_r, rec_r = st.WorldBatch(n)
    st.SetWorldCapacity(0)  # back to the exact first pass of a ComputeBatch
    off_0, rec_0 = st.WorldBatch(n)
    for off, rec in ((off_t, rec_t), (off_r, rec_r), (off_0, rec_0)):
        assert np.array_equal(off, off_a) and rec.tobytes() == rec_a.tobytes()
    # into an array the caller keeps: a view of its head, nothing behind the records touched
    keep = np.zeros(len(rec_a) + 5, host.WORLD_DTYPE)
    keep["reserved"][len(rec_a):] = 77
    off_k, rec_k = st.WorldBatch(n, out=keep)
    assert rec_k.base is keep and np.array_equal(off_k, off_a) and rec_k.tobytes() == rec_a.tobytes()
    assert (keep["reserved"][len(rec_a):] == 77).all()
    off_s, rec_small = st.WorldBatch(n, out=np.zeros(3, host.WORLD_DTYPE))  # too small: a fresh array
    assert rec_small.tobytes() == rec_a.tobytes()
    with pytest.raises(ValueError, match="WORLD_DTYPE"):
        st.WorldBatch(n, out=np.zeros(10, np.int32))
    # a caller's stream
    s = torch.cuda.Stream(device=dev)
    off_s, rec_s = st.WorldBatch(n, stream=s.cuda_stream)
    assert np.array_equal(off_s, off_a) and rec_s.tobytes() == rec_a.tobytes()
    # world.pointcloud on device records equals it on the restatement's records
    cam = {"intrinsic": {"fx": float(np.float32(cfg.focal)), "fy": float(np.float32(cfg.focal)),
                         "u0": float(np.float32(cfg.camera_center_x)), "v0": float(np.float32(cfg.camera_center_y))},
           "extrinsic": {"baseline": float(np.float32(cfg.baseline))}}
    C = st.GetRealCols()
    got = world.pointcloud(rec_a[off_a[1]:off_a[2]], (256, 512), (data[1].alpha_ground, data[1].vhor), cam, C)
    want = world.pointcloud(wr.records_of(cfg, data[1], maps[1]), (256, 512), (data[1].alpha_ground, data[1].vhor),
                            cam, C)
    for key in want:
        assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), key
    assert len(got["points"]) > 0 and len(got["ground_semantics"]) > 0
    st.close()


def test_host_class_refusals():
    case = helpers.build_case("drn_d_22_unary", 128, 256, 32, seed=3, n_images=2)
    cfg = case["cfg"]
    st = host.Stixels()
    st.SetConfig(cfg)
    st.Initialize(max_batch=2)
    with pytest.raises(ValueError, match="there are none"):
        st.WorldBatch(1)
    big, seg = _dev(case["disparity"]), _dev(case["segmentation"])
    road = [(f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground) for f in case["frames"]]
    st.ComputeBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), road[:1])
    for bad in (0, 2):
        with pytest.raises(ValueError, match="n_images outside"):
            st.WorldBatch(bad)
    for bad in (-1, -5, 10 ** 9):
        with pytest.raises(ValueError, match="SetWorldCapacity"):
            st.SetWorldCapacity(bad)
    assert len(st.WorldBatch(1)[1]) > 0
    st.close()
    # no camera centre: Get3DVertices' refusal
    import dataclasses
    st = host.Stixels()
    st.SetConfig(dataclasses.replace(cfg, camera_center_x=-1.0))
    st.Initialize(max_batch=2)
    st.ComputeBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), road)
    with pytest.raises(ValueError, match="Camera parameters are not set"):
        st.WorldBatch(2)
    st.close()


def test_world_is_refused_after_a_gather():
    """ComputeBatchGather leaves this rank's shard in d_stixels: WorldBatch refuses it like RenderBatch (a fresh
    child process with a one-rank RCCL communicator, tests/world_gather_child.py)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(root, "tests", "world_gather_child.py")],
                         capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert out.returncode == 0 and "WORLD_GATHER_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
