"""CPU tests of bench.py's output contract: ONE compact JSON line on stdout (< 4 KB, the keys the driver and
the judge read), the complete object in a file beside it, and the `--gpus N` launcher that relays a child's
line (no GPU: the result object is a fake with the shape -- and more than the size -- of a real --full run)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

REQUIRED = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "verify_all_ok",
            "value_pruning_off", "value_floor_families", "lut_fused_repaired")
ROOFLINE = ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "kernel_ms",
            "algorithmic_bytes_per_image", "traffic_source", "from_committed_profile")


def fake_result(bloat=1):
    """What main() hands to emit() after a --full run, with every free-text / list field inflated."""
    families = {f"family_{i}": {"images_per_s": 9000.0 + i, "evaluated_frac": 0.2, "verify": {"ok": True},
                                "what": "x" * 300 * bloat} for i in range(8)}
    return {
        "metric": "images/s on 1024x2048x128-disp column DP", "value": 11293.32617738783, "unit": "images/s",
        "n_gpus": 1, "steps": 20, "warmup": 5, "ms_per_step": 5.66706380341202, "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f32+i32", "data": "synthetic",
        "config": {"workload": "C2/C3: 64 frames/GPU of 1024x2048, 128 disparity bins, 19 classes + 2 offset "
                               "channels, preset drn_d_22_unary (unary), input family scene, JoinColumns + prepare "
                               "+ DP + back-trace, device-resident in/out" + " pad" * 40 * bloat,
                   "batch_per_gpu": 64, "rows": 1024, "cols": 2048, "max_dis": 128, "preset": "drn_d_22_unary",
                   "family": "scene", "parallelism": "single GPU"},
        "roofline": {"bound": "hbm", "achieved": 226.02, "peak": 8000.0, "unit": "GB/s", "frac": 0.02825,
                     "traffic": 16397243776.0, "kernel": "k_dp_unary_fast " + "y" * 200 * bloat, "kernel_ms": 4.398,
                     "kernel_ms_how": "HIP events " + "h" * 100 * bloat,
                     "algorithmic_bytes_per_image": 15532032, "traffic_source": "profiles/r06_traffic.json",
                     "from_committed_profile": True, "measured_hbm_frac": 0.466, "note": "n" * 400 * bloat},
        "valu": {"issue_frac": 0.839, "formula": "f" * 500 * bloat},
        "prune": {"evaluated_frac": 0.15, "how": "h" * 400 * bloat},
        "kernel_ms": {"prepare_ms": 0.96, "dp_ms": 4.398, "backtrace_ms": 0.14},
        "value_incl_d2h": 8169.2, "single_frame": {"images_per_s": 2500.0, "ms_per_frame": 0.4},
        "timed_blocks": {"count": 71, "seconds": [0.1133] * 71 * bloat},
        "verify": {"frames_checked": [0, 31, 32, 63], "ok": True},
        "value_spread": {"what": "s" * 2000 * bloat},
        "variants": {"families": families, "what": "v" * 5000 * bloat},
        "value_incl_instances": 11036.4,
        "value_floor_families": {"images_per_s": 8856.29, "family": "cityscapes_like",
                                 "families_measured": [f"family_{i}" for i in range(8)]},
        "value_pruning_off": 3051.13, "lut_fused_repaired": 0,
        "cpu_baseline": {"value": 3.864, "unit": "images/s", "cores": 16, "kind": "port",
                         "sample": "24 x one 1024x2048x128 frame " + "c" * 100 * bloat,
                         "single_thread_value": 0.245},
        "other_model": {"preset": "drn_d_38_pairwise", "images_per_s": 4481.0, "dp_ms": 11.3, "pruning_off": 1800.0,
                        "single_frame_ms": 1.5},
        "distinct_frames": 64, "verify_all_ok": True,
        "verified": [{"what": "w" * 80, "ok": True} for _ in range(40 * bloat)],
    }


@pytest.mark.parametrize("bloat", [1, 20])
def test_compact_line_is_short_strict_json_with_the_required_keys(bloat, tmp_path, capsys):
    out = fake_result(bloat)
    assert len(json.dumps(out)) > 4 * bench.COMPACT_LIMIT   # (the shape that broke the driver's parse in round 5: 29 KB)
    line = bench.emit(out, str(tmp_path / "bench_full.json"))
    printed = capsys.readouterr().out
    assert printed == line + "\n" and "\n" not in line
    assert len(line.encode()) < 4096
    d = json.loads(line, parse_constant=lambda c: pytest.fail(f"non-strict JSON constant {c}"))
    for k in REQUIRED:
        assert k in d, k
    for k in ROOFLINE:
        assert k in d["roofline"], k
    assert d["config"]["workload"] and "model" not in d["config"]
    assert d["roofline"]["from_committed_profile"] is True
    assert set(d["cpu_baseline"]) == {"value", "unit", "cores", "kind", "sample"}
    assert d["value"] == pytest.approx(out["value"], rel=1e-4)
    full = json.load(open(tmp_path / "bench_full.json"))
    assert full["variants"] and full["verified"] and full["timed_blocks"]["seconds"]
    assert os.path.join(ROOT, d["full"]) and os.path.samefile(os.path.join(ROOT, d["full"]), tmp_path / "bench_full.json")


def test_compact_line_of_a_default_run_without_the_optional_parts():
    out = fake_result()
    for k in ("variants", "value_spread", "other_model", "value_incl_instances", "valu", "value_floor_families"):
        out.pop(k)
    out["cpu_baseline"] = None
    d = json.loads(bench.compact_line(out))
    assert d["value_floor_families"] is None and d["cpu_baseline"] is None and d["lut_fused_repaired"] == 0


def _run_bench(args, child):
    env = dict(os.environ, IS_BENCH_CHILD_CMD=json.dumps(child))
    env.pop("WORLD_SIZE", None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                          timeout=120, env=env, cwd=ROOT)


def test_gpus_n_without_a_launcher_starts_a_child_and_relays_its_line():
    """`python bench.py --gpus 2` with no WORLD_SIZE: the parent (no torch import, no HIP) starts the ranks as a
    child process and makes rank 0's JSON line its own LAST line, whatever the child printed after it (RCCL's
    banner at exit); the child's exit code is the parent's."""
    line = json.dumps({"metric": "images/s on 1024x2048x128-disp column DP", "value": 2.0, "n_gpus": 2})
    child = [sys.executable, "-c",
             "import sys; print('rank noise'); print(%r); print('RCCL banner after the line'); sys.exit(0)" % line]
    out = _run_bench(["--gpus", "2", "--steps", "3"], child)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[-1] == line and lines[0] == "rank noise" and "RCCL banner after the line" in lines
    assert json.loads(lines[-1])["n_gpus"] == 2
    # a failing child: its code comes back, nothing is invented
    out = _run_bench(["--gpus", "2"], [sys.executable, "-c", "import sys; print('boom'); sys.exit(7)"])
    assert out.returncode == 7 and out.stdout.strip().splitlines() == ["boom"]


def test_gpus_n_launcher_command_is_torch_distributed_run():
    """The command the parent would start (read from the source: nothing is launched here)."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert '"-m", "torch.distributed.run", "--nnodes=1"' in src and '"--master-addr", "127.0.0.1"' in src
    assert "os.exec" not in src            # a child process, never a re-exec


def _fake_workload(B, C, S, seed=5):
    """What dump_outputs reads of a bench Workload, on the CPU: a [B][C][S] Section batch with a terminator in
    every column and garbage behind it (the format leaves those entries unspecified)."""
    import types
    import numpy as np
    import torch
    from instance_stixels_amd.config import SECTION_DTYPE
    rng = np.random.default_rng(seed)
    rec = np.zeros((B, C, S), SECTION_DTYPE)
    for f in SECTION_DTYPE.names:
        rec[f] = rng.integers(0, 1000, rec.shape) if rec[f].dtype == np.int32 else rng.random(rec.shape)
    n = rng.integers(0, S, (B, C))
    rec["type"][np.arange(S) == n[..., None]] = -1
    rec["type"][np.arange(S) < n[..., None]] = rng.integers(0, 3, (B, C, S))[np.arange(S) < n[..., None]]
    d = torch.from_numpy(rec.view(np.int32).reshape(B, C, S, 8).copy())
    return types.SimpleNamespace(B=B, C=C, S=S, torch=torch), d, rec, n


def test_dump_outputs_writes_the_sections_as_float32_up_to_each_terminator(tmp_path):
    import numpy as np
    wl, d, rec, n = _fake_workload(3, 5, 7)
    info = bench.dump_outputs(wl, d, str(tmp_path))
    assert info["images"] == [0, 1, 2] and info["bytes"] <= bench.DUMP_LIMIT
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(f + ".npy" for f in info["files"])
    np.testing.assert_array_equal(np.load(tmp_path / "stixels_per_column.npy"), n)
    valid = np.arange(7) <= n[..., None]
    for f in rec.dtype.names:
        a = np.load(tmp_path / f"sections_{f}.npy")
        assert a.dtype == np.float32 and a.shape == (3, 5, 7)
        np.testing.assert_array_equal(a[valid], rec[f][valid].astype(np.float32))
        assert not a[~valid].any()


def test_dump_outputs_of_a_large_batch_is_a_fixed_sample_under_the_limit(tmp_path):
    """Per image 256 columns x 200 sections (the bench's 1024x2048 frames): 64 images are 100 MB, more than the
    limit; the sample of images is the same in every run."""
    import numpy as np
    wl, d, rec, n = _fake_workload(64, 256, 200)
    a = bench.dump_outputs(wl, d, str(tmp_path / "a"))
    b = bench.dump_outputs(wl, d, str(tmp_path / "b"))
    assert a["images"] == b["images"] and 1 <= len(a["images"]) < 64 and a["bytes"] <= bench.DUMP_LIMIT
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) == a["bytes"]
    k = np.asarray(a["images"])
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "images.npy"), k)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "sections_vB.npy")[:, :, 0], rec["vB"][k, :, 0])
    for f in a["files"]:
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f"{f}.npy"), np.load(tmp_path / "b" / f"{f}.npy"))
