"""Many parameter sets on one resident batch: Stixels::SweepBatch against what a hyper-parameter search could do
before it (GPU box).

Prints one JSON line per preset and batch size, at 1024x2048x128, 8 sets, 64 and 8 frames (4 distinct) by default.
Every figure is the host clock around calls that end in a synchronisation, after a warm-up; median [min, max] over
--iters rounds, all forms in turn in the same rounds:
  (a) sweep_ms          one SweepBatch of all sets, with instances; the results stay on the device
      sweep_fetch_ms    the same plus SweepSections of every set: everything (b) brings to the host
  (b) batches_ms        one ComputeBatch (with instances) on each of 8 objects initialised beforehand, one per set
                        (null when the device cannot hold 8 contexts of this batch size)
  (c) reinit_ms         per set SetConfig + Finish + Initialize + ComputeBatch on ONE object: what a search has to do
                        without the sweep (--reinit-iters rounds, it allocates the whole scratch per set)
  (d) recluster_ms      ReclusterBatch of set 1 of the sweep with its own clustering parameters (the mappings
                        delivered to the host) against
      recompute_ms      the ComputeBatch of object 1 of (b): the same Sections, candidates and labels
      recluster_device_ms   ReclusterBatch without the mappings and a synchronisation: the device's share
`sweep_below_batches` = (b) median - (a) median exceeds the larger of the two spreads (max - min), the rule of
DESIGN.md section 10d; `recluster_below_recompute` likewise.  The sweep is verified first: set k's Sections and
mappings of the first --verify frames against object k of (b).
For kernel times run `rocprofv3 --kernel-trace --stats -- python tools/sweep_timing.py --device-only --n 8`
(`--device-only batches`: the ComputeBatch calls of (b) alone, for the same kernels outside a sweep).

    python tools/sweep_timing.py [--rows 1024 --cols 2048 --max-dis 128 --n 64,8 --sets 8 --iters 20]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def stat(ts):
    import numpy as np
    return [round(float(np.median(ts)), 3), round(float(np.min(ts)), 3), round(float(np.max(ts)), 3)]


def below(np, fast, slow):
    spread = max(max(fast) - min(fast), max(slow) - min(slow))
    return bool(np.median(slow) - np.median(fast) > spread)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--cols", type=int, default=2048)
    ap.add_argument("--max-dis", type=int, default=128)
    ap.add_argument("--n", default="64,8", help="frames per batch, comma separated")
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reinit-iters", type=int, default=3)
    ap.add_argument("--verify", type=int, default=2)
    ap.add_argument("--presets", default="drn_d_22_unary,drn_d_38_pairwise")
    ap.add_argument("--device-only", nargs="?", const="sweep", choices=("sweep", "batches"),
                    help="for a profiler run: only SweepBatch and ReclusterBatch, or only the ComputeBatch calls of (b)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import helpers
    from instance_stixels_amd import host, make_config, synthetic
    if not torch.cuda.is_available():
        sys.exit("sweep_timing.py needs a GPU")
    rows, cols, D = a.rows, a.cols, a.max_dis
    dev = torch.device("cuda", 0)
    fields = ("prior_weight", "disparity_weight", "segmentation_weight", "instance_weight", "eps", "min_pts",
              "size_filter")
    for preset in a.presets.split(","):
        base = make_config(preset, rows, cols, D)
        # the sets: the weights spread around the preset's as a search samples them, the clustering changed in half
        factors = [(1.0, 1.0), (0.1, 1.0), (1.0, 30.0), (0.3, 3.0), (3.0, 0.3), (0.5, 10.0), (2.0, 1.0), (1.0, 0.1)]
        cfgs = []
        for k in range(a.sets):
            fs, fd = factors[k % len(factors)]
            ov = dict(segmentation_weight=base.segmentation_weight * fs, disparity_weight=base.disparity_weight * fd)
            if k % 2:
                ov.update(eps=base.eps * 0.7, min_pts=base.min_pts + 1, size_filter=max(1, base.size_filter // 2))
            cfgs.append(make_config(preset, rows, cols, D, **ov))
        sets = [tuple(getattr(c, f) for f in fields) for c in cfgs]
        frames = [synthetic.make_frame(base, seed=7 + i, n_slabs=12, offset_scale=1.0) for i in range(4)]
        for n in [int(x) for x in a.n.split(",")]:
            big = torch.from_numpy(np.stack([frames[i % 4].disparity for i in range(n)])).to(dev)
            seg = torch.from_numpy(np.stack([frames[i % 4].segmentation for i in range(n)])).to(dev)
            road = [(f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground)
                    for f in (frames[i % 4] for i in range(n))]
            args = (base.pairwise, big.data_ptr(), seg.data_ptr(), road)
            out = {"preset": preset, "shape": [rows, cols, D], "n": n, "sets": a.sets, "iters": a.iters}
            sw = host.Stixels()
            sw.SetConfig(base)
            sw.Initialize(max_batch=n)
            recl = cfgs[1]
            if a.device_only == "batches":
                sw.close()
                objs = []
                for c in cfgs:
                    objs.append(host.Stixels())
                    objs[-1].SetConfig(c)
                    objs[-1].Initialize(max_batch=n)
                for _ in range(a.iters):
                    for st in objs:
                        st.ComputeBatch(*args)
                for st in objs:
                    st.close()
                print(json.dumps(out), flush=True)
                continue
            if a.device_only:
                for _ in range(a.iters):
                    sw.SweepBatch(*args, sets)
                    sw.SelectSweepSet(1)
                    sw.ReclusterBatch(recl.eps, recl.min_pts, recl.size_filter, with_mapping=False)
                torch.cuda.synchronize()
                sw.close()
                print(json.dumps(out), flush=True)
                continue
            objs = []
            try:
                for c in cfgs:
                    st = host.Stixels()
                    objs.append(st)
                    st.SetConfig(c)
                    st.Initialize(max_batch=n)
            except RuntimeError as e:
                out["batches_refused"] = str(e)[:120]
                for st in objs:
                    st.close()
                objs = []
            # verify: set k of the sweep against object k
            sw.SweepBatch(*args, sets)
            v = min(a.verify, n)
            same = bool(objs)
            for k, st in enumerate(objs):
                data, maps = st.ComputeBatch(*args)
                sdata, smaps = sw.SweepSections(k)
                same = same and all(helpers.sections_equal(data[i].sections, sdata[i].sections) and
                                    maps[i] == smaps[i] for i in range(v))
            out["sweep_identical_to_batches"] = same if objs else None
            re = host.Stixels()   # (c): one object, configured anew per set
            re.SetConfig(base)
            re.Initialize(max_batch=n)
            t = {key: [] for key in ("sweep_ms", "sweep_fetch_ms", "batches_ms", "reinit_ms", "recluster_ms",
                                     "recompute_ms", "recluster_device_ms")}
            for it in range(-2, a.iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sw.SweepBatch(*args, sets)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for k in range(a.sets):
                    sw.SweepSections(k)
                t2 = time.perf_counter()
                for st in objs:
                    st.ComputeBatch(*args)
                t3 = time.perf_counter()
                sw.SelectSweepSet(1)
                sw.ReclusterBatch(recl.eps, recl.min_pts, recl.size_filter)
                t4 = time.perf_counter()
                if objs:
                    objs[1].ComputeBatch(*args)
                t5 = time.perf_counter()
                sw.ReclusterBatch(recl.eps, recl.min_pts, recl.size_filter, with_mapping=False)
                torch.cuda.synchronize()
                t6 = time.perf_counter()
                if it >= 0:
                    t["sweep_ms"].append((t1 - t0) * 1e3)
                    t["sweep_fetch_ms"].append((t2 - t0) * 1e3)
                    if objs:
                        t["batches_ms"].append((t3 - t2) * 1e3)
                        t["recompute_ms"].append((t5 - t4) * 1e3)
                    t["recluster_ms"].append((t4 - t3) * 1e3)
                    t["recluster_device_ms"].append((t6 - t5) * 1e3)
                if 0 <= it < a.reinit_iters:
                    t0 = time.perf_counter()
                    for c in cfgs:
                        re.SetConfig(c)
                        re.Finish()
                        re.Initialize(max_batch=n)
                        re.ComputeBatch(*args)
                    t["reinit_ms"].append((time.perf_counter() - t0) * 1e3)
            for key, ts in t.items():
                out[key] = stat(ts) if ts else None
            if objs:
                out["sweep_below_batches"] = below(np, t["sweep_ms"], t["batches_ms"])
                out["sweep_fetch_below_batches"] = below(np, t["sweep_fetch_ms"], t["batches_ms"])
                out["recluster_below_recompute"] = below(np, t["recluster_ms"], t["recompute_ms"])
            for st in objs + [sw, re]:
                st.close()
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
