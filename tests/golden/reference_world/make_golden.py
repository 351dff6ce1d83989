"""Generates tests/golden/reference_world/reference_world.npz -- the pin of instance_stixels_amd/world.py
against the reference tooling's 3-D view.

Reads a checkout of the reference at generation time only (REFERENCE, default: beside this repository); only
the resulting vectors (data) are committed.

What is executed from the reference: `pointcloud` and `compute3d` of
tools/visualization/clustering_visualization.py, as they stand there.  The module cannot be imported as a whole
(its top level needs cv2 and cityscapesscripts), so the two function definitions are cut out of the parsed source
(ast) and executed in a namespace that holds ONLY numpy and copy, as tests/golden/reference_python/make_golden.py
does for the reader and the clustering twin.

Per case (small frames, CPU only):
  oracle DP -> Section[], twin-oracle clustering -> {(column, section): label}
  -> the list of per-column dicts in the shape the reference's read_stixel_file returns (type, vB, vT, disparity,
     class, cost, instance_mean_x/y, and instance_label by its rule -- label + class*1000 for 0 <= label < 1000,
     else -1 -- for the instance candidates only), FILLED FROM THE BINARY SECTIONS: SaveStixels prints six
     significant digits, and this pin is bit-exact
  -> reference pointcloud(stixels, (rows, cols), max_dis, (alpha_ground, vhor), camera) -> its seven arrays.
The reference raises ValueError on a zero disparity; the generator asserts that its cases have none (no object
stixel with disparity 0, no ground stixel with vB or vT on the groundplane row).

    python tests/golden/reference_world/make_golden.py
"""
import ast
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REFERENCE = os.environ.get("REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
REF = os.path.join(REFERENCE, "tools", "visualization", "clustering_visualization.py")
WANTED = ("pointcloud", "compute3d")
KEYS = ("points3d", "points", "pixels", "ground_patches3d", "ground_semantics", "object_semantics", "instances")

CASES = [  # preset, rows, cols, max_dis, seed, n_slabs, overrides
    ("drn_d_22_unary", 256, 1024, 64, 5, 14, dict(size_filter=12, eps=23.89408, min_pts=4)),
    ("drn_d_38_pairwise", 256, 1024, 64, 9, 18, dict(size_filter=8, eps=18.822322, min_pts=3)),
    ("drn_d_22_pairwise", 128, 512, 32, 2, 8, dict(size_filter=6, eps=30.0, min_pts=2)),
]


def reference_functions():
    tree = ast.parse(open(REF).read())
    picked = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANTED]
    assert sorted(n.name for n in picked) == sorted(WANTED)
    ns = {"np": np, "copy": copy}
    exec(compile(ast.Module(body=picked, type_ignores=[]), REF, "exec"), ns)
    return ns


def camera_of(cfg):
    """The dictionary the reference's compute3d reads, from the configuration's camera (float32 values, as the
    library holds them)."""
    f = float(np.float32(cfg.focal))
    return {"intrinsic": {"fx": f, "fy": f, "u0": float(np.float32(cfg.camera_center_x)),
                          "v0": float(np.float32(cfg.camera_center_y))},
            "extrinsic": {"baseline": float(np.float32(cfg.baseline))}}


def stixel_dicts(sections, mapping):
    """[realcols][max_sections] Sections + {(column, section): label} -> what read_stixel_file returns."""
    import helpers
    out = []
    for c in range(sections.shape[0]):
        column = []
        for i in range(helpers.n_sections(sections[c])):
            s = sections[c, i]
            entry = {"type": int(s["type"]), "vB": int(s["vB"]), "vT": int(s["vT"]),
                     "disparity": float(s["disparity"]), "class": int(s["semantic_class"]),
                     "cost": float(s["cost"]), "instance_mean_x": float(s["instance_meanx"]),
                     "instance_mean_y": float(s["instance_meany"])}
            if entry["type"] == 1 and entry["class"] >= 11:  # an instance candidate (StixelsKernels.cu:926)
                label = mapping.get((c, i), -1)
                entry["instance_label"] = label + entry["class"] * 1000 if 0 <= label < 1000 else -1
            column.append(entry)
        out.append(column)
    return out


def main():
    import helpers
    from oracle import oracle
    from instance_stixels_amd import synthetic
    fns = reference_functions()
    out = {}
    for k, (preset, rows, cols, D, seed, n_slabs, ov) in enumerate(CASES):
        case = helpers.build_case(preset, rows, cols, D, seed=seed, **ov)
        cfg = case["cfg"]
        frame = synthetic.make_frame(cfg, seed=seed, n_slabs=n_slabs, offset_scale=1.0)
        case["frames"] = [frame]
        case["disparity"] = frame.disparity[None]
        case["segmentation"] = frame.segmentation[None]
        ref = helpers.run_oracle(case)
        secs = ref["sections"]
        vhor = int(case["vhor"][0])
        mapping = {}
        for cls in range(8):
            n = int(ref["inst_per_class"][cls])
            if n == 0:
                continue
            lab = oracle.cluster_instances(ref["inst_centerofmass"][cls][:n], ref["inst_core"][cls][:n], cfg.eps,
                                           cfg.min_pts)
            for (u, v), l in zip(ref["inst_indices"][cls][:n].tolist(), lab.tolist()):
                mapping[(u, v)] = l
        stixels = stixel_dicts(secs, mapping)
        flat = [s for col in stixels for s in col]
        assert not any(s["type"] == 1 and s["disparity"] == 0 for s in flat), f"case {k}: object at disparity 0"
        assert not any(s["type"] == 0 and vhor in (s["vB"], s["vT"]) for s in flat), f"case {k}: ground at vhor"
        groundplane = (float(np.float32(frame.alpha_ground)), vhor)
        pc = fns["pointcloud"](stixels, (rows, cols), D, groundplane, camera_of(cfg))
        assert sorted(pc) == sorted(KEYS)
        n_cand = sum("instance_label" in s for s in flat)
        assert len(pc["instances"]) == n_cand and n_cand > 0 and (pc["instances"] >= 0).any()
        print(f"case {k}: {preset} {rows}x{cols}x{D}: {len(flat)} stixels, {len(pc['points'])} object, "
              f"{len(pc['ground_semantics'])} ground, {n_cand} candidates, "
              f"{len(np.unique(pc['instances'][pc['instances'] >= 0]))} instances")
        out[f"c{k}_sections"] = secs.view(np.int32).reshape(*secs.shape, 8)
        out[f"c{k}_mapping"] = np.array([[u, v, l] for (u, v), l in sorted(mapping.items())], np.int32).reshape(-1, 3)
        out[f"c{k}_meta"] = np.array([rows, cols, D, vhor, int(cfg.column_step)], np.int32)
        out[f"c{k}_camera"] = np.array([cfg.focal, cfg.baseline, cfg.camera_center_x, cfg.camera_center_y,
                                        frame.alpha_ground], np.float32)
        out[f"c{k}_preset"] = np.frombuffer(preset.encode(), np.uint8)
        for key in KEYS:
            out[f"c{k}_{key}"] = pc[key]
    out["n_cases"] = np.array(len(CASES), np.int32)
    path = os.path.join(HERE, "reference_world.npz")
    np.savez_compressed(path, **out)
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
