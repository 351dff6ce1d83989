"""GPU tests of the block of records the walk holds across rows (k_unary_path).

The walk keeps the 64 records of its last full step in the lanes across rows: a row whose first block is the held one
loads no record, and takes record vT + 1 from the lane that owned the previous hop's vB (unless vT = 64 s + 64, where
vT + 1 belongs to the block above).  The LUT networks of a step run once per distinct fn of its live lanes, so the cases
also hold first steps with many and with one fn.  Every case runs one batch through the tile path
(IS_UNARY_PATH=0), the walk (=1) and a distrusted walk (=3) into zero-filled Section buffers, compares the three outputs
as whole int32 arrays -- no tolerance -- and every column of the walk's output with the CPU oracle.

Coverage.  Each case first asserts on the CPU, from the oracle's Sections and the joined disparities alone, that it
contains what it is there for (COVER below; a hop goes from visited row vT to row vB - 1, the first step of a row vT
holds the candidates vB = 64 ((vT - 1) >> 6) + 1 .. vT, and a candidate's fn is the floor of the mean joined disparity
of rows vB .. vT, counted only where it is at least 1e-3 away from an integer):
  same    a hop whose next row starts in the block this row started in ((vB - 2) >> 6 == (vT - 1) >> 6)
  lower   a hop into a lower block
  vb1     a hop with vB = 64 k + 1, k >= 1: the next row is 64 k, its first block the one below
  vt0     a visited row vT = 64 k, k >= 1: record vT + 1 lies outside the row's first block
  fn5     a first step with at least five distinct fn
  fn1     a first step of at least two candidates with exactly one fn
Counts per input (hops same | lower | vb1 | vt0 rows | first steps fn5 | fn1), seeds chosen on the CPU:
  scene 256x512x128 (2 frames, seed 400)        1415 |  384 | 13 | 13 |  656 |  580
  iid_noise 256x512x128 (400)                   3606 |  384 | 56 | 56 | 1784 | 1083
  homogeneous 256x512x128 (414)                  290 |  237 |  1 |  1 |   92 |  130
  noisy_disparity 256x512x128 (400)             1444 |  384 | 16 | 16 |  687 |  197
  scene 256x512x128, invalid_disparity = 0      1414 |  384 | 17 | 17 |  649 |  589
  scene 200x256x64 (400)                         498 |  192 |  3 |  3 |  321 |  263
  scene 136x128x48, median join (403)            188 |   64 |  1 |  1 |   71 |  104
  scene 64x128x32 (400): one block               116 |    0 |  0 |  0 |  119 |    3
  scene 256x512x256 (400)                       1415 |  384 | 13 | 13 |  963 |  583
  max_sections 2 / 3 / 5 (scene 256x512x128)     128 / 256 / 476 | 0 / 0 / 36 | 0 / 0 / 9 | 0 / 0 / 9 | 24 / 35 / 47 |
                                                 232 / 349 / 529 (chains of one or two Sections never leave the top block)
  two calls: scene (410), then iid_noise (420)  3598 |  384 | 45 | 45 | 1831 | 1125 (the second call's input)
On the device (a counting build of the walk that the default build does not carry), 16 scene frames of the bench shape:
69.4 full steps per column, 45.8 of them on the held block, 56.6 rows, 45.4 of them with record vT + 1 from a lane.
"""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

ALL = ("same", "lower", "vb1", "vt0", "fn5", "fn1")


def _core(case, monkeypatch, env, max_batch=None):
    from instance_stixels_amd.core import Core
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return Core(case["params"], case["lut"], case["odr"], max_batch=max_batch or len(case["frames"]))
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _run(core, case):
    """One unary call without instance outputs into zero-filled Sections: ([n][C][S][8] int32, joined [n][C][H])."""
    import torch
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
    core.compute_ptr(joined.data_ptr(), seg.data_ptr(), case["gf"], case["ng"], case["ig"], case["vhor"], False, n,
                     sections.data_ptr(), None, None, None, stream)
    torch.cuda.synchronize(dev)
    return sections.cpu().numpy(), joined.cpu().numpy()


def _family_case(family, H, W, D, n, seed, **ov):
    from instance_stixels_amd import synthetic
    from oracle import oracle
    base = helpers.build_case("drn_d_22_unary", H, W, D, seed=5, n_images=1, **ov)
    cfg = base["cfg"]
    frames = [synthetic.make_frame(cfg, seed=seed + i, family=family) for i in range(n)]
    ground = [oracle.host_ground(cfg, f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground) for f in frames]
    return dict(base, frames=frames, gf=np.stack([g[0] for g in ground]), ng=np.stack([g[1] for g in ground]),
                ig=np.stack([g[2] for g in ground]), vhor=np.array([g[3] for g in ground], np.int32),
                disparity=np.stack([f.disparity for f in frames]),
                segmentation=np.stack([f.segmentation for f in frames]))


def _oracle_all(case):
    """The CPU oracle's Sections [n][C][S] and joined disparities [n][C][H] of every image."""
    refs = [helpers.run_oracle(case, image=i) for i in range(len(case["frames"]))]
    return refs


def coverage(case, refs):
    """The counts of COVER from the oracle's Sections and the joined disparities (see the module docstring)."""
    cfg = case["cfg"]
    H, D, S = int(cfg.rows), int(cfg.max_dis), int(case["params"].max_sections)
    inv = float(case["params"].invalid_disparity)
    cnt = dict.fromkeys(ALL, 0)
    for ref in refs:
        for c in range(cfg.realcols):
            col = ref["sections"][c]
            ns = helpers.n_sections(col)
            d = np.asarray(ref["joined"][c], np.float64)
            ok = (d != inv) if inv >= 0 else np.ones(H, bool)
            ps = np.concatenate([[0.0], np.cumsum(np.where(ok, d, 0.0))])
            pv = np.concatenate([[0], np.cumsum(ok)])
            rows = [H - 1]
            for i in range(ns):
                vT, vB = int(col["vT"][i]), int(col["vB"][i])
                assert vT == rows[-1]
                if vB == 0:
                    break
                if (vB - 2) >> 6 == (vT - 1) >> 6:
                    cnt["same"] += 1
                elif vB >= 2:
                    cnt["lower"] += 1
                if vB % 64 == 1 and vB > 1:
                    cnt["vb1"] += 1
                if i < S - 1:   # (the row of the last possible Section is still visited)
                    rows.append(vB - 1)
            for vT in rows:
                if vT % 64 == 0 and vT > 0:
                    cnt["vt0"] += 1
                lo = 64 * ((vT - 1) >> 6) + 1
                if vT < 1:
                    continue
                vB = np.arange(lo, vT + 1)
                nv = pv[vT + 1] - pv[vB]
                mean = np.where(nv > 0, (ps[vT + 1] - ps[vB]) / np.maximum(nv, 1), 0.0)
                mean = np.clip(mean, 0.0, None)
                sure = np.abs(mean - np.round(mean)) >= 1e-3
                fn = np.minimum(np.floor(mean), D - 1)
                if len(np.unique(fn[sure])) >= 5:
                    cnt["fn5"] += 1
                if len(vB) >= 2 and sure.all() and len(np.unique(fn)) == 1:
                    cnt["fn1"] += 1
    return cnt


def _check(case, monkeypatch, need):
    from instance_stixels_amd.core import SECTION_DTYPE
    refs = _oracle_all(case)
    cnt = coverage(case, refs)
    print("coverage", cnt)
    missing = [k for k in need if cnt[k] == 0]
    assert not missing, f"the case does not contain {missing}: {cnt}"
    out = {}
    for mode, repaired in (("0", 0), ("1", 0), ("3", 1)):
        core = _core(case, monkeypatch, dict(IS_UNARY_PATH=mode))
        try:
            out[mode], joined = _run(core, case)
            assert core.unary_path() == (0 if mode == "0" else 1, repaired)
        finally:
            core.close()
    for mode in ("1", "3"):
        diff = np.argwhere((out[mode] != out["0"]).any(axis=(2, 3)))
        assert diff.size == 0, f"IS_UNARY_PATH={mode}: Sections differ from the tile path in (image, column) " \
                               f"{diff[:8].tolist()}"
    n, C, S = out["1"].shape[:3]
    got = dict(sections=out["1"].view(SECTION_DTYPE).reshape(n, C, S), joined=joined)
    for img, ref in enumerate(refs):
        errs = helpers.compare(ref, got, img, case["cfg"], check_tables=False)
        assert not errs, "\n".join(errs[:5])
    return out["1"]


# (family, H, W, D, frames, seed, overrides, what the case must contain)
CASES = [
    ("scene", 256, 512, 128, 2, 400, {}, ALL),
    ("iid_noise", 256, 512, 128, 2, 400, {}, ALL),
    ("homogeneous", 256, 512, 128, 2, 414, {}, ALL),
    ("noisy_disparity", 256, 512, 128, 2, 400, {}, ALL),
    ("scene", 256, 512, 128, 2, 400, dict(invalid_disparity=0.0), ALL),
    ("scene", 200, 256, 64, 2, 400, {}, ALL),                        # H % 64 != 0
    ("scene", 136, 128, 48, 2, 403, dict(median_join=True), ALL),    # H % 32 != 0
    ("scene", 64, 128, 32, 2, 400, {}, ("same", "fn1")),             # one block: every hop stays in it
    ("scene", 256, 512, 256, 2, 400, {}, ALL),
]


@pytest.mark.parametrize("family,H,W,D,n,seed,ov,need", CASES,
                         ids=[f"{c[0]}-{c[1]}x{c[2]}x{c[3]}{'-inv' if 'invalid_disparity' in c[6] else ''}"
                              for c in CASES])
def test_walk_reuse_on_inputs(family, H, W, D, n, seed, ov, need, monkeypatch):
    _check(_family_case(family, H, W, D, n, seed, **ov), monkeypatch, need)


@pytest.mark.parametrize("S,seed", [(2, 400), (3, 400), (5, 400)])
def test_walk_reuse_stops_at_max_sections(S, seed, monkeypatch):
    """A small max_sections: the chain ends with the block still held; the last visited row only writes its pairs."""
    case = _family_case("scene", 256, 512, 128, 2, seed)
    case["params"].max_sections = S
    need = ALL if S == 5 else ("same", "fn5", "fn1")   # (one or two Sections stay in the top block)
    _check(case, monkeypatch, need)


def test_walk_reuse_does_not_leak_between_calls(monkeypatch):
    """Two calls on one context, the second on other frames: the held block and the row cache of a column start
    empty in every call (and in every column: the columns of a call differ)."""
    first = _family_case("scene", 256, 512, 128, 2, 410)
    second = _family_case("iid_noise", 256, 512, 128, 2, 420)
    refs = _oracle_all(second)
    cnt = coverage(second, refs)
    assert all(cnt[k] > 0 for k in ALL), cnt
    tile_core = _core(second, monkeypatch, dict(IS_UNARY_PATH="0"))
    try:
        tile, _ = _run(tile_core, second)
    finally:
        tile_core.close()
    for mode, repaired in (("1", 0), ("3", 2)):
        core = _core(first, monkeypatch, dict(IS_UNARY_PATH=mode))
        try:
            _run(core, first)
            got, _ = _run(core, second)
            assert core.unary_path() == (1, repaired)
            assert np.array_equal(got, tile), f"IS_UNARY_PATH={mode}: the second call differs from the tile path"
        finally:
            core.close()
