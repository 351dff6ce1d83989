"""Road estimation + stixel computation of a resident batch: the host-side chain against the device-resident one
(GPU box).

    legacy   RoadEstimation::ComputeBatch (lines to the host, line choice there, one synchronisation) +
             Stixels::ComputeBatch (BatchGround on the host, staging upload, DP)
    device   RoadEstimation::ComputeBatchDevice + Stixels::ComputeBatchRoad on one stream: line choice and ground
             model on the device, no synchronisation before the one that delivers the Sections

Before anything is timed the two chains run once through the Python views at the timed size, and the line says how many
road records are bitwise equal and how many Sections differ.  Both then run inside the host library as a C++ caller's loop would (ish_time_road_chain: outputs reused, host clock around
calls that end in a synchronisation), alternating, `--repeats` blocks of `--iters` calls each after a warm-up call per
block; the spread is taken over the block medians.  Cases: 64 resident frames of 1024 x 2048 x 128, unary and pairwise,
and 8 frames.  Also the host time of the ground model alone (SetRoadParameters + GetGroundModel per frame: what
BatchGround computes), which is the share of the legacy chain no launch hides.

A tree without the device chain (the parent of the change that added it) is measured with --legacy-only: there the
legacy chain is the sum of ire_compute_batch and ish_time_compute_batch, both synchronous; on a tree that has
ish_time_road_chain the same sum is printed beside the chain's own figure, so that the two methods can be compared.

    python tools/ground_device_timing.py [--iters 10 --repeats 5] [--legacy-only] [--root TREE]

Prints one JSON line per case.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--legacy-only", action="store_true")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="the tree whose libraries are measured (default: this one)")
ap.add_argument("--cases", default="unary:64,pairwise:64,unary:8,pairwise:8")
ARGS = ap.parse_args()
ROOT = os.path.abspath(ARGS.root)
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

ROWS, COLS, D = 1024, 2048, 128


def stats(blocks):
    import numpy as np
    med = [float(np.median(b)) * 1e3 for b in blocks]
    return dict(ms_median=round(float(np.median(med)), 3), ms_block_medians=[round(m, 3) for m in med],
                ms_spread=round(max(med) - min(med), 3), ms_min=round(min(min(b) for b in blocks) * 1e3, 3))


def main():
    import numpy as np
    import torch
    import helpers
    from instance_stixels_amd import host
    if not torch.cuda.is_available():
        sys.exit("ground_device_timing.py needs a GPU")
    L = host.lib()
    have_chain = hasattr(L, "ish_time_road_chain") and not ARGS.legacy_only
    dev = torch.device("cuda", 0)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    for spec in ARGS.cases.split(","):
        mode, n = spec.split(":")
        n, pairwise = int(n), mode == "pairwise"
        preset = "drn_d_38_pairwise" if pairwise else "drn_d_22_unary"
        case = helpers.build_case(preset, ROWS, COLS, D, seed=1, n_images=min(n, 8))
        k = len(case["frames"])
        cfg = case["cfg"]
        d_big = torch.from_numpy(np.stack([case["disparity"][i % k] for i in range(n)])).to(dev)
        d_seg = torch.from_numpy(np.ascontiguousarray(np.stack([case["segmentation"][i % k] for i in range(n)]),
                                                      np.int32)).to(dev)
        d_road = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        d_status = torch.zeros((n,), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        f0 = case["frames"][0]
        fb = np.array([f0.vhor_image, f0.camera_tilt, f0.camera_height, f0.alpha_ground], np.float32)
        st = host.Stixels()
        st.SetConfig(cfg)
        st.Initialize(max_batch=n)
        re_ = host.RoadEstimation()
        re_.Initialize(cfg.camera_center_y * ROWS / 1024, cfg.baseline, cfg.focal, ROWS, COLS, D)
        road, ok = re_.ComputeBatch(d_big.data_ptr(), n)
        road = [r if o else tuple(fb) for r, o in zip(road, ok)]
        rp = np.ascontiguousarray(road, np.float32).reshape(n, 4)

        def verify():
            """the two chains once through the Python views, at the size that is timed: the roads, the status bytes
            and the Sections of the device chain against the legacy chain's"""
            re_.ComputeBatchDevice(d_big.data_ptr(), n, d_road.data_ptr(), d_status.data_ptr(), fb)
            torch.cuda.synchronize()
            new, _, road_d, status = st.ComputeBatchRoad(pairwise, n, d_big.data_ptr(), d_seg.data_ptr(),
                                                         d_road.data_ptr(), d_status.data_ptr(), with_instances=False)
            old, _ = st.ComputeBatch(pairwise, d_big.data_ptr(), d_seg.data_ptr(), road, with_instances=False)
            equal_roads = sum(np.array([a], host.ROAD_PARAMETERS_DTYPE).tobytes() ==
                              np.array([tuple(b)], host.ROAD_PARAMETERS_DTYPE).tobytes() for a, b in zip(road_d, road))
            differ = total = 0
            for a, b in zip(new, old):
                ta, tb = a.sections["type"] == -1, b.sections["type"] == -1
                na, nb = ta.argmax(axis=1), tb.argmax(axis=1)
                total += int(np.maximum(na, nb).sum())
                for c in np.flatnonzero(na != nb):
                    differ += abs(int(na[c]) - int(nb[c]))
                m = np.minimum(na, nb)
                live = np.arange(a.sections.shape[1])[None, :] < m[:, None]
                va = a.sections.view(np.int32).reshape(*a.sections.shape, 8)
                vb = b.sections.view(np.int32).reshape(*b.sections.shape, 8)
                differ += int(((va != vb).any(axis=2) & live).sum())
            return dict(device_status_ok=int(sum(x == 1 for x in status)), roads_bitwise_equal=int(equal_roads),
                        sections_differ=differ, sections=total)

        def chain(device_chain):
            each = np.zeros(ARGS.iters, np.float64)
            rc = L.ish_time_road_chain(st._h, re_._h, int(device_chain), int(pairwise), n, vp(d_big.data_ptr()),
                                       vp(d_seg.data_ptr()), vp(d_road.data_ptr()), vp(d_status.data_ptr()),
                                       vp(fb.ctypes.data), ARGS.iters, 0, vp(each.ctypes.data))
            if rc != 0:
                sys.exit("ish_time_road_chain: " + L.ish_last_error().decode())
            return each

        def legacy_sum():
            """the two synchronous halves timed one after the other (works on a tree without ish_time_road_chain)"""
            out = np.zeros(n, host.ROAD_PARAMETERS_DTYPE)
            okb = np.zeros(n, np.uint8)
            L.ire_compute_batch(re_._h, vp(d_big.data_ptr()), n, vp(out.ctypes.data), vp(okb.ctypes.data), None)
            each = np.zeros(ARGS.iters, np.float64)
            for i in range(ARGS.iters):
                t0 = time.perf_counter()
                L.ire_compute_batch(re_._h, vp(d_big.data_ptr()), n, vp(out.ctypes.data), vp(okb.ctypes.data), None)
                each[i] = time.perf_counter() - t0
            s = ctypes.c_double()
            L.ish_time_compute_batch(st._h, int(pairwise), n, vp(d_big.data_ptr()), vp(d_seg.data_ptr()),
                                     vp(rp.ctypes.data), ARGS.iters, 0, ctypes.byref(s))
            return each + s.value, float(np.median(each)) * 1e3, s.value * 1e3

        def ground_host():
            each = np.zeros(ARGS.iters, np.float64)
            for i in range(ARGS.iters):
                t0 = time.perf_counter()
                for r in road:
                    st.SetRoadParameters(int(r[0]), float(r[1]), float(r[2]), float(r[3]))
                    st.GetGroundModel()
                each[i] = time.perf_counter() - t0
            return each

        checked = verify() if have_chain else None
        if have_chain:
            L.ish_time_road_chain.argtypes = [vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, ci, ci, vp]
        res = dict(legacy_sum=[], legacy=[], device=[], ground_host=[])
        parts = []
        for _ in range(ARGS.repeats):   # alternating: the versions share whatever else the host is doing
            s, road_ms, stixels_ms = legacy_sum()
            res["legacy_sum"].append(s)
            parts.append((round(road_ms, 3), round(stixels_ms, 3)))
            if have_chain:
                res["legacy"].append(chain(0))
                res["device"].append(chain(1))
            res["ground_host"].append(ground_host())
        line = {"tree": os.path.basename(ROOT) or ROOT, "shape": [ROWS, COLS, D], "mode": mode, "n": n,
                "iters": ARGS.iters, "repeats": ARGS.repeats, "frames_with_a_road": int(sum(ok)),
                "legacy_sum": stats(res["legacy_sum"]), "legacy_sum_parts_ms(road, stixels)": parts,
                "ground_model_on_host": stats(res["ground_host"])}
        if have_chain:
            line["device_against_legacy"] = checked
            line["legacy"] = stats(res["legacy"])
            line["device"] = stats(res["device"])
            line["device_minus_legacy_ms"] = round(line["device"]["ms_median"] - line["legacy"]["ms_median"], 3)
        print(json.dumps(line), flush=True)
        st.close()
        re_.close()
        del d_big, d_seg
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
