"""Generates tests/golden/reference_python_disp/instance_disparity_reference_python.npz -- the pin of f10
(is_cluster_instance_disparity / Stixels::ClusterInstanceDisparityBatch) on the reference's own Python.

BUILD-CONTAINER ONLY: reads the reference checkout (REFERENCE, default /root/reference) at generation time; only the
resulting arrays (data) are committed and travel to the GPU box.

What is executed from the reference, byte for byte as it stands there, cut out of the parsed source (ast) as
tests/golden/reference_python/make_golden.py does:
  read_stixel_file                 tools/visualization/clustering_visualization.py:73-116
  get_disparity_instance_centers   :794-819
  assign_instances                 :894-960   (with use_instance_disparity = "from_gt")
  add_instance_disparity           :996-1022
  compute_instance_disparity       :1024-1049
in a namespace of numpy, copy and sklearn's DBSCAN.  numpy goes in through a proxy that adds `float = float`:
compute_instance_disparity says np.float, which numpy 2 no longer has.  The per-class masks come from
load_instance_mask (tools/visualization/cityscapes_instance_loader.py:32-71) RESTATED below on an array: reading the
PNG with PIL is the only thing replaced.

Pipeline per case (the shapes of the f1 pin, CPU only):
  oracle DP -> Section[]; Stixels::SaveStixels -> text; the reference's read_stixel_file(text) -> stixels
  ground truth: instance_eval_reference.synth_gt of the instance image of the 2-D twin labels, restricted to
      0..65535, plus seeded patches over chosen stixels (see `patches`)
  disparity_u8: the frame's disparity rounded, a few percent of the pixels 0, the patches' own values
  compute_instance_disparity -> add_instance_disparity -> assign_instances
The generator REFUSES to write a fixture that a wrong implementation could satisfy (see `conditions`).

    python tests/golden/reference_python_disp/make_golden.py
"""
import ast
import contextlib
import copy
import io
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REFERENCE = os.environ.get("REFERENCE", "/root/reference")
REF = os.path.join(REFERENCE, "tools/visualization/clustering_visualization.py")
WANTED = ("read_stixel_file", "get_disparity_instance_centers", "assign_instances", "add_instance_disparity",
          "compute_instance_disparity")
LABEL_IDS = (24, 25, 26, 27, 28, 31, 32, 33)
MARGIN = 1e-4   # of tests/golden/reference_python/make_golden.py: fp32 against sklearn's binary64

CASES = [  # preset, rows, cols, max_dis, seed, n_slabs, overrides, seed of the ground truth, grey levels per pixel of disparity
    # (the last two chosen until `conditions` holds; an 8-bit disparity file has a scale of its own, and at 32
    # disparities against eps = 30 the depth separates nothing below 4 levels per pixel)
    ("drn_d_22_unary", 256, 1024, 64, 5, 14, dict(size_filter=12, eps=23.89408, min_pts=4), 65, 1),
    ("drn_d_38_pairwise", 256, 1024, 64, 9, 18, dict(size_filter=8, eps=18.822322, min_pts=3), 69, 1),
    ("drn_d_22_unary", 128, 512, 32, 2, 8, dict(size_filter=6, eps=30.0, min_pts=2), 62, 4),
]


class _NumpyWithFloat:
    """numpy plus the alias the reference still uses."""
    float = float

    def __getattr__(self, name):
        return getattr(np, name)


def reference_functions():
    from sklearn.cluster import DBSCAN
    tree = ast.parse(open(REF).read())
    picked = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANTED]
    assert sorted(n.name for n in picked) == sorted(WANTED)
    ns = {"np": _NumpyWithFloat(), "copy": copy, "DBSCAN": DBSCAN}
    exec(compile(ast.Module(body=picked, type_ignores=[]), REF, "exec"), ns)
    return ns


def load_instance_mask(mask):
    """cityscapes_instance_loader.py:32-71 for *_instanceIds.png with return_trainIds, on the array PIL would read."""
    mask = np.asarray(mask)
    mask_both = mask * (mask > 1000)
    r, c = mask_both.shape
    train_ids = np.array([11, 12, 13, 14, 15, 16, 17, 18])
    classes = np.array(LABEL_IDS)
    masks_per_class = np.empty((len(classes), r, c))
    for idx, (id_, train_id) in enumerate(zip(classes, train_ids)):
        mask_class = mask_both * (mask_both >= id_ * 1000) * (mask_both < (id_ + 1) * 1000)
        non_zero = mask_class != 0
        mask_class[non_zero] = mask_class[non_zero] % (id_ * 1000) + train_id * 1000
        masks_per_class[idx] = mask_class
    return masks_per_class


def patches(gt, disp, secs, rows, cols, rng):
    """Seeded corner cases over stixels of an instance class, in place: (0) two new instances side by side, one with
    an even count of 10 | 11 (median 10.5), one at 20: the stixel's median is 15.25; (1) stuff only: the stixel's
    median is 0 and it takes no part; (2) a new instance whose disparities are all 0: a key without a median."""
    import render_reference as rr
    C = secs.shape[0]
    w = cols // C
    cand = [(c, i) for c in range(C) for i in range(rr.column_count(secs[c]))
            if 11 <= secs[c, i]["semantic_class"] <= 18 and secs[c, i]["vT"] - secs[c, i]["vB"] >= 3]
    rng.shuffle(cand)
    for n, (c, i) in enumerate(cand[:9]):
        s = secs[c, i]
        L = LABEL_IDS[int(s["semantic_class"]) - 11]
        top, bot = rows - 1 - int(s["vT"]), rows - 1 - int(s["vB"])
        box, dbox = gt[top:bot + 1, c * w:c * w + w], disp[top:bot + 1, c * w:c * w + w]
        kind = n % 3
        if kind == 0:
            box[:, :w // 2] = L * 1000 + 900 + n
            box[:, w // 2:] = L * 1000 + 950 + n
            dbox[:, :w // 2] = 10 + (np.arange(dbox[:, :w // 2].size).reshape(dbox[:, :w // 2].shape) % 2)
            dbox[:, w // 2:] = 20
        elif kind == 1:
            box[...] = 7
        else:
            box[...] = L * 1000 + 800 + n
            dbox[...] = 0


def conditions(stixels, labelled, key_median, eps, min_pts, size_filter):
    """What the reference itself met, from its own answers: the counts the fixture is refused without."""
    import instance_disparity_reference as idr
    k = dict(key_half=0, stixel_quarter=0, excluded=0, key_empty=0, z_matters=0)
    present = key_median >= 0
    k["key_half"] = int((present & (key_median * 2 % 2 == 1)).sum())
    k["key_empty"] = int((present & (key_median == 0)).sum())
    for col in stixels:
        for s in col:
            if s["class"] > 10:
                m = float(s["instance_disparity"])
                k["stixel_quarter"] += (m * 4) % 2 == 1
                k["excluded"] += m == 0
    worst = np.inf
    for cls in range(11, 19):
        pts = [(s, l) for col, lcol in zip(stixels, labelled) for s, l in zip(col, lcol)
               if s["class"] == cls and s["instance_disparity"] != 0]
        if not pts:
            continue
        X = np.array([[s["instance_mean_x"], s["instance_mean_y"], s["instance_disparity"]] for s, _ in pts], np.float64)
        size = np.array([s["vT"] - s["vB"] + 1 for s, _ in pts])
        lab3 = np.array([l["instance_label"] for _, l in pts])
        # margin: no pair on the eps boundary
        d2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
        worst = min(worst, np.abs(d2 - eps ** 2).min() / eps ** 2)
        # no small point with its two nearest cores in different clusters within the margin
        flat = X.copy()
        flat[:, 2] = 0
        lab2 = idr.cluster3(flat, size >= size_filter, eps, min_pts)
        core = np.nonzero((size >= size_filter) & ((d2[:, size >= size_filter] <= eps ** 2).sum(1) >= min_pts))[0]
        for p in np.nonzero(size < size_filter)[0]:
            if core.size < 2:
                break
            order = np.argsort(d2[p, core], kind="stable")[:2]
            a, b = core[order]
            if lab3[a] != lab3[b]:
                worst = min(worst, abs(d2[p, a] - d2[p, b]) / eps ** 2)
        from oracle import oracle
        k["z_matters"] += not oracle.same_partition(np.where(lab3 >= 0, lab3 % 1000, -1), lab2)
    return k, worst


def main():
    import helpers
    import instance_disparity_reference as idr
    import instance_eval_reference as ir
    import render_reference as rr
    from oracle import oracle
    from instance_stixels_amd import host, synthetic
    fns = reference_functions()
    out = {}
    for k, (preset, rows, cols, D, seed, n_slabs, ov, gt_seed, levels) in enumerate(CASES):
        case = helpers.build_case(preset, rows, cols, D, seed=seed, **ov)
        cfg = case["cfg"]
        frame = synthetic.make_frame(cfg, seed=seed, n_slabs=n_slabs, offset_scale=1.0)
        case["frames"] = [frame]
        case["disparity"] = frame.disparity[None]
        case["segmentation"] = frame.segmentation[None]
        ref = helpers.run_oracle(case)
        secs = ref["sections"]
        C, S = secs.shape
        mapping = {}
        for cls in range(8):
            n = int(ref["inst_per_class"][cls])
            if n == 0:
                continue
            lab = oracle.cluster_instances(ref["inst_centerofmass"][cls][:n], ref["inst_core"][cls][:n], cfg.eps,
                                           cfg.min_pts)
            for (u, v), l in zip(ref["inst_indices"][cls][:n].tolist(), lab.tolist()):
                mapping[(u, v)] = l
        inst = rr.render(secs[None], rows, cols, [mapping])[2]
        gt = np.clip(ir.synth_gt(inst, seed=gt_seed)[0], 0, 65535).astype(np.int32)
        rng = np.random.default_rng(gt_seed + 1)
        disp = np.clip(np.rint(np.nan_to_num(frame.disparity) * levels), 0, 255).astype(np.uint8)
        disp[rng.random(disp.shape) < 0.04] = 0
        patches(gt, disp, secs, rows, cols, rng)

        st = host.Stixels()
        st.SetConfig(cfg)
        st.PrecomputeHost()
        data = host.StixelsData(secs, rows, cols, C, S, D, 8, 19, frame.alpha_ground, int(case["vhor"][0]))
        with tempfile.TemporaryDirectory() as tmp:
            fa = os.path.join(tmp, "a.stixels")
            st.SaveStixels(data, {}, frame.alpha_ground, int(case["vhor"][0]), fa)
            with contextlib.redirect_stdout(io.StringIO()):
                stixels, _ = fns["read_stixel_file"](fa)
        st.close()
        assert len(stixels) == C and all(len(col) == rr.column_count(secs[c]) for c, col in enumerate(stixels))
        assert all(s["type"] == 1 for col in stixels for s in col if s["class"] > 10), "a candidate that is no object"

        masks = load_instance_mask(gt)
        cluster_config = dict(eps=float(cfg.eps), min_size=int(cfg.min_pts), size_filter=int(cfg.size_filter),
                              use_instance_disparity="from_gt")
        with contextlib.redirect_stdout(io.StringIO()):
            image = fns["compute_instance_disparity"](disp, masks)
            with_disp = fns["add_instance_disparity"](stixels, image)
            labelled = fns["assign_instances"](with_disp, cluster_config)

        # ---- the reference's answers as arrays
        key_median = np.full(idr.KEYS, -1.0)          # -1: the key is absent
        for ci in range(8):
            for v in np.unique(masks[ci][masks[ci] > 1000]).astype(np.int64).tolist():
                vals = np.unique(image[masks[ci] == v])
                assert vals.size == 1
                key_median[ci * 1000 + v % 1000] = vals[0]
        stixel_median = np.full((C, S), -1.0)          # -1: no stixel
        ref_labels = np.full((C, S), -2, np.int32)     # -2: the reference gave the stixel no label
        for c in range(C):
            for i, (s, l) in enumerate(zip(with_disp[c], labelled[c])):
                stixel_median[c, i] = s["instance_disparity"]
                if "instance_label" in l:
                    ref_labels[c, i] = l["instance_label"]
        cond, worst = conditions(with_disp, labelled, key_median, float(cfg.eps), int(cfg.min_pts), int(cfg.size_filter))
        print(f"case {k}: {preset} {rows}x{cols}x{D}: {int((key_median >= 0).sum())} keys, "
              f"{int((ref_labels >= -1).sum())} stixels of an instance class, {int((ref_labels >= 0).sum())} labelled; "
              f"{cond}, margin {worst:.3e}")
        for name, n in cond.items():
            assert n >= 1, f"case {k}: {name} = 0: pick another seed"
        assert worst > MARGIN, f"case {k}: a pair or a small point within {MARGIN} of a decision boundary ({worst})"
        out[f"c{k}_sections"] = secs.view(np.int32).reshape(C, S, 8)
        out[f"c{k}_gt"] = gt.astype(np.uint16)
        out[f"c{k}_disparity_u8"] = disp
        out[f"c{k}_ref_key_median"] = key_median
        out[f"c{k}_ref_stixel_median"] = stixel_median
        out[f"c{k}_ref_labels"] = ref_labels
        out[f"c{k}_meta"] = np.array([rows, cols, D, seed, n_slabs, int(cfg.size_filter), int(cfg.min_pts)], np.int32)
        out[f"c{k}_eps"] = np.array(cfg.eps, np.float64)
        out[f"c{k}_cond"] = np.array([cond[n] for n in sorted(cond)], np.int32)
    out["n_cases"] = np.array(len(CASES), np.int32)
    out["cond_names"] = np.frombuffer(",".join(sorted(cond)).encode(), np.uint8)
    np.savez_compressed(os.path.join(HERE, "instance_disparity_reference_python.npz"), **out)
    print("written", os.path.join(HERE, "instance_disparity_reference_python.npz"))


if __name__ == "__main__":
    main()
