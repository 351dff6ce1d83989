"""The 3-D stixel world of a batch from the device (Stixels::WorldBatch) against the host composition that
existed before it (GPU box).

Prints one JSON line per DP mode's preset, at 1024x2048x128 and 64 frames by default.  Every figure is the host
clock around calls that end in a synchronisation, after a warm-up; median [min, max] over --iters rounds.
  (a) the export, every form a caller can reach, copy to the host included:
      view_ms     C++ Stixels::WorldBatchView: the records left in the object's pinned buffer
      reuse_ms    C++ Stixels::WorldBatch(n, world) into a World that keeps its capacity
      value_ms    C++ Stixels::WorldBatch(n) by value (fresh pages per call), released inside the timed region
      py_out_ms   Python host.Stixels.WorldBatch(n, out=array kept between the rounds) (= ish_world_batch +
                  ish_world_records: one copy out of pinned memory)
      py_fresh_ms Python host.Stixels.WorldBatch(n) into a fresh array per call
  (c) host_ms: the baseline -- per frame Get3DVertices(out[i]) plus one instance_stixels[i] lookup per stixel into
      a vector of the same records per frame, in C++ (tools/world_baseline.cpp, built here with g++ on first use),
      the frames over --threads host threads, the per-frame vectors keeping their capacity between the rounds; the
      clock stops when the threads have joined.  concat_ms is what copying those vectors into ONE array adds.
      The C++ forms of (a) and (c) are timed in the same call, in turn; `faster_<form>` = (c) median - (a) median
      exceeds the larger of the two spreads (max - min).
  (b) device_ms: the device work alone -- is_stixel_world on the Sections of the same ComputeBatch, --iters
      launches queued back to back between two synchronisations -- and the GB/s of the bytes it must move (32 B
      read per slot scanned up to and including the terminator, 96 B written per record) against the 6.3 TB/s
      achievable HBM bandwidth.  The launches rotate over --rotate output buffers (default 6, > 500 MB together) so
      that the stores cannot stay in the 256 MB last-level cache from one launch to the next; device_same_buffer_ms
      is the same with one buffer.  For kernel times run the tool under
      `rocprofv3 --kernel-trace --stats -- python tools/world_timing.py --device-only` (k_world,
      k_count_sections, k_scan_counts).
The records of the first frame are verified against the host composition first (tests/world_reference.py for the
layout, Get3DVertices for the vertices), and the C++ rounds compare all frames.

    python tools/world_timing.py [--rows 1024 --cols 2048 --max-dis 128 --n 64 --iters 10 --threads 16]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

HBM_GBS = 6300.0


def baseline_lib():
    """tools/libworld_baseline.so, built from world_baseline.cpp when it is missing or older than its source."""
    here = os.path.dirname(os.path.abspath(__file__))
    src, so = os.path.join(here, "world_baseline.cpp"), os.path.join(here, "libworld_baseline.so")
    libdir = os.path.join(ROOT, "instance_stixels_amd", "lib")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared",
                        "-I" + os.path.join(ROOT, "include"), src, "-L" + libdir, "-lInstanceStixels", "-lis_core",
                        "-Wl,-rpath," + libdir, "-pthread", "-o", so], check=True)
    L = ctypes.CDLL(so)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.wt_time_world.argtypes = [vp, ci, ci, vp, vp, vp, ci, ci, vp, vp, vp, vp, vp,
                                ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ci)]
    return L


def stat(ts):
    import numpy as np
    return [round(float(np.median(ts)), 3), round(float(np.min(ts)), 3), round(float(np.max(ts)), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--cols", type=int, default=2048)
    ap.add_argument("--max-dis", type=int, default=128)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--rotate", type=int, default=6, help="output buffers the device-only launches rotate over")
    ap.add_argument("--presets", default="drn_d_22_unary,drn_d_38_pairwise")
    ap.add_argument("--device-only", action="store_true", help="only the device work (for a profiler run)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import helpers
    import world_reference as wr
    from instance_stixels_amd import core, host
    if not torch.cuda.is_available():
        sys.exit("world_timing.py needs a GPU")
    rows, cols, D, n = a.rows, a.cols, a.max_dis, a.n
    dev = torch.device("cuda", 0)
    for preset in a.presets.split(","):
        case = helpers.build_case(preset, rows, cols, D, seed=1, n_images=min(n, 8),
                                  size_filter=10 if preset.endswith("unary") else 8)
        cfg, k = case["cfg"], min(n, 8)
        big = torch.from_numpy(np.stack([case["disparity"][i % k] for i in range(n)])).to(dev)
        seg = torch.from_numpy(np.stack([case["segmentation"][i % k] for i in range(n)])).to(dev)
        road = [(f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground)
                for f in (case["frames"][i % k] for i in range(n))]
        st = host.Stixels()
        st.SetConfig(cfg)
        st.Initialize(max_batch=n)
        data, maps = st.ComputeBatch(cfg.pairwise, big.data_ptr(), seg.data_ptr(), road, with_instances=True)
        offsets, records = st.WorldBatch(n)
        want0 = wr.records_of(cfg, data[0], maps[0])
        want0["vertices"] = st.Get3DVertices(data[0]).reshape(-1, 12)
        wr.assert_records_equal(records[:offsets[1]], want0)
        out = {"preset": preset, "shape": [rows, cols, D], "n": n, "iters": a.iters, "records": int(offsets[-1]),
               "record_MB": round(int(offsets[-1]) * 96 / 1e6, 2), "frame0_verified": True}

        # (b) the device work alone, on the Sections of that call
        secs = np.stack([d.sections for d in data])
        C, S = secs.shape[1:]
        used = np.array([helpers.n_sections(secs[i, c]) for i in range(n) for c in range(C)])
        d_sec = torch.from_numpy(secs.view(np.int32).reshape(n, C, S, 8)).to(dev)
        inst = np.full((n, C, S), -1, np.int32)
        for i, m in enumerate(maps):
            for (c, s), l in m.items():
                inst[i, c, s] = l
        d_inst = torch.from_numpy(inst).to(dev)
        cap = int(offsets[-1])
        d_counts = torch.zeros(n * C, dtype=torch.int32, device=dev)
        d_offsets = torch.zeros(n * C + 1, dtype=torch.int32, device=dev)
        d_totals = torch.zeros(n, dtype=torch.int32, device=dev)
        d_worlds = [torch.zeros(cap * 24, dtype=torch.int32, device=dev) for _ in range(max(a.rotate, 1))]
        alpha, vhor = [d.alpha_ground for d in data], [d.vhor for d in data]

        def launch(k=0):
            core.stixel_world_ptr(alpha, vhor, d_sections=d_sec.data_ptr(), d_section_instance=d_inst.data_ptr(),
                                  n_images=n, realcols=C, max_sections=S, rows=rows,
                                  column_step=int(cfg.column_step), focal=cfg.focal, baseline=cfg.baseline,
                                  camera_center_x=cfg.camera_center_x, camera_center_y=cfg.camera_center_y,
                                  capacity=cap, d_counts=d_counts.data_ptr(), d_offsets=d_offsets.data_ptr(),
                                  d_frame_totals=d_totals.data_ptr(), d_world=d_worlds[k % len(d_worlds)].data_ptr())

        for k in range(len(d_worlds)):
            launch(k)
        torch.cuda.synchronize()
        same = all(w.cpu().numpy().view(core.WORLD_DTYPE).tobytes() == records.tobytes() for w in d_worlds[:2])
        nbytes = 32 * int((used + 1).sum()) + 96 * cap
        for key, rotate in (("device", True), ("device_same_buffer", False)):
            reps = []
            for _ in range(5):
                t0 = time.perf_counter()
                for k in range(a.iters):
                    launch(k if rotate else 0)
                torch.cuda.synchronize()
                reps.append((time.perf_counter() - t0) * 1e3 / a.iters)
            ms = float(np.median(reps))
            out[key + "_ms"] = round(ms, 4)
            out[key + "_ms_min"] = round(min(reps), 4)
            out[key + "_GBps"] = round(nbytes / ms / 1e6, 1)
        out.update(device_bytes=nbytes, device_buffers=len(d_worlds),
                   device_pct_of_hbm=round(100 * out["device_GBps"] / HBM_GBS, 2),
                   device_records_identical=bool(same))
        del d_worlds

        if not a.device_only:
            # the Python forms (ish_world_batch + ish_world_records)
            keep = np.empty(cap, host.WORLD_DTYPE)
            py = {"py_out_ms": [], "py_fresh_ms": []}
            for it in range(-2, a.iters):
                t0 = time.perf_counter()
                o1, r1 = st.WorldBatch(n, out=keep)
                t1 = time.perf_counter()
                o2, r2 = st.WorldBatch(n)
                t2 = time.perf_counter()
                if it >= 0:
                    py["py_out_ms"].append((t1 - t0) * 1e3)
                    py["py_fresh_ms"].append((t2 - t1) * 1e3)
                del r2
            assert r1.base is keep and r1.tobytes() == records.tobytes()
            # the C++ forms and the baseline, in turn in one call
            rp = np.ascontiguousarray(road, np.float32).reshape(n, 4)
            t = {k: np.zeros(a.iters) for k in ("view_ms", "reuse_ms", "value_ms", "host_ms", "concat_ms")}
            nrec, ident = ctypes.c_int64(), ctypes.c_int()
            rc = baseline_lib().wt_time_world(st._h, int(bool(cfg.pairwise)), n, big.data_ptr(), seg.data_ptr(),
                                              rp.ctypes.data, a.iters, a.threads, *[t[k].ctypes.data for k in t],
                                              ctypes.byref(nrec), ctypes.byref(ident))
            assert rc == 0 and nrec.value == cap
            t.update({k: np.array(v) for k, v in py.items()})
            for k, v in t.items():
                out[k] = stat(v)
            out["host_plus_concat_ms"] = stat(t["host_ms"] + t["concat_ms"])
            host_med, host_spread = np.median(t["host_ms"]), t["host_ms"].max() - t["host_ms"].min()
            for k in ("view_ms", "reuse_ms", "value_ms", "py_out_ms", "py_fresh_ms"):
                spread = max(host_spread, t[k].max() - t[k].min())
                out["faster_" + k[:-3]] = bool(host_med - np.median(t[k]) > spread)
            out.update(host_threads=a.threads, all_frames_identical=bool(ident.value))
        st.close()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
