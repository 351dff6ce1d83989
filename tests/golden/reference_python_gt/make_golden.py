"""Generates tests/golden/reference_python_gt/assign_gt_reference_python.npz -- the pin of f8
(is_assign_instances_gt / Stixels::AssignInstancesGTBatch) on the reference's own Python.

BUILD-CONTAINER ONLY: reads the reference checkout (REFERENCE, default /root/reference) at generation time; only
the resulting vectors (data) are committed and travel to the GPU box.

What is executed from the reference, byte for byte as it stands there, cut out of the parsed sources (ast) as
tests/golden/reference_python/make_golden.py does:
  assign_instances_gt   tools/visualization/clustering_visualization.py:846-891
  load_instance_mask    tools/visualization/cityscapes_instance_loader.py:32-71
each in a namespace that holds ONLY what it needs: numpy and copy for the first, numpy and PIL's Image for the
second.  numpy goes in through a proxy that adds `int = int`: the function says np.int, which numpy 2 no longer has.

Pipeline per case (small frames, CPU only):
  oracle DP -> Section[] and the oracle twin's cluster labels
  render_reference.render        -> the instance image of those
  ground truth: instance_eval_reference.synth_gt of it, restricted to 0..65535 (a 16-bit PNG), plus seeded
      patches over chosen stixels that make the vote's corner cases frequent: two values with exactly the same
      count, a dozen instances none of which reaches a tenth of the stixel, group ids (labelId*1000)
  PIL writes <tmp>/x_instanceIds.png (I;16), the reference's load_instance_mask reads it back
  the reference's assign_instances_gt(stixels, masks) -> instance_label of every stixel of an instance class
The generator REFUSES to write a fixture the vote could satisfy trivially (see `need`).

    python tests/golden/reference_python_gt/make_golden.py
"""
import ast
import copy
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REFERENCE = os.environ.get("REFERENCE", "/root/reference")
REF_ASSIGN = os.path.join(REFERENCE, "tools/visualization/clustering_visualization.py")
REF_LOADER = os.path.join(REFERENCE, "tools/visualization/cityscapes_instance_loader.py")
LABEL_IDS = (24, 25, 26, 27, 28, 31, 32, 33)

CASES = [  # preset, rows, cols, max_dis, seed, n_slabs, overrides
    ("drn_d_22_unary", 256, 1024, 64, 5, 14, dict(size_filter=12, eps=23.89408, min_pts=4)),
    ("drn_d_38_pairwise", 256, 1024, 64, 9, 18, dict(size_filter=8, eps=18.822322, min_pts=3)),
    ("drn_d_22_unary", 192, 1028, 32, 2, 16, dict(size_filter=6, eps=30.0, min_pts=2)),   # cols % 8 == 4
]


class _NumpyWithInt:
    """numpy plus the alias the reference still uses."""
    int = int

    def __getattr__(self, name):
        return getattr(np, name)


def _cut(path, name, ns):
    tree = ast.parse(open(path).read())
    picked = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name]
    assert len(picked) == 1, name
    exec(compile(ast.Module(body=picked, type_ignores=[]), path, "exec"), ns)
    return ns[name]


def reference_functions():
    from PIL import Image
    assign = _cut(REF_ASSIGN, "assign_instances_gt", {"np": _NumpyWithInt(), "copy": copy})
    load = _cut(REF_LOADER, "load_instance_mask", {"np": np, "Image": Image})
    return assign, load


def patches(gt, secs, rows, cols, rng):
    """Seeded corner cases over stixels of an instance class, in place."""
    import render_reference as rr
    C = secs.shape[0]
    w = cols // C
    cand = [(c, i) for c in range(C) for i in range(rr.column_count(secs[c]))
            if 11 <= secs[c, i]["semantic_class"] <= 18 and secs[c, i]["vT"] - secs[c, i]["vB"] >= 3]
    rng.shuffle(cand)
    for n, (c, i) in enumerate(cand[:len(cand) * 2 // 3]):
        s = secs[c, i]
        L = LABEL_IDS[int(s["semantic_class"]) - 11]
        top, bot = rows - 1 - int(s["vT"]), rows - 1 - int(s["vB"])
        box = gt[top:bot + 1, c * w:c * w + w]
        kind = n % 4
        if kind == 0:      # two values with exactly the same count: left half | right half
            a, b = rng.choice(np.arange(0, 40), 2, replace=False)
            box[:, :w // 2] = L * 1000 + int(a) if a else 7       # (a == 0: background against an instance)
            box[:, w // 2:2 * (w // 2)] = L * 1000 + int(b)
            box[:, 2 * (w // 2):] = 8
        elif kind == 1:    # 12..16 instances in confetti: none reaches a tenth of the stixel
            ids = L * 1000 + rng.choice(np.arange(1, 200), int(rng.integers(12, 17)), replace=False)
            box[...] = ids[np.arange(box.size).reshape(box.shape) % len(ids)]
        elif kind == 2:    # the group id of the class
            box[...] = L * 1000
        else:              # an instance of ANOTHER class covers most of it: background wins
            other = LABEL_IDS[(int(s["semantic_class"]) - 11 + 3) % 8]
            box[: max(1, box.shape[0] * 3 // 4)] = other * 1000 + 5


def stats(stixels, masks, labelled, rows, w):
    """The corner cases the reference itself met, counted from its masks and its answers."""
    k = dict(instance=0, labelled=0, rule=0, background=0, ties=0, group=0)
    for c, column in enumerate(stixels):
        for i, s in enumerate(column):
            if s["class"] < 11:
                continue
            k["instance"] += 1
            got = labelled[c][i]["instance_label"]
            k["labelled"] += got >= 0
            px = masks[s["class"] - 11][rows - 1 - s["vT"]:rows - s["vB"], c * w:c * w + w].astype(np.int64)
            counts = np.bincount(px.ravel())
            top2 = np.sort(counts)[-2:]
            k["ties"] += len(top2) == 2 and top2[0] == top2[1]
            win = int(counts.argmax())
            k["background"] += win == 0
            k["rule"] += win > 1000 and got == -1
            k["group"] += win > 1000 and win % 1000 == 0 and got >= 0
    return k


def main():
    import helpers
    import instance_eval_reference as ir
    import render_reference as rr
    from PIL import Image
    from oracle import oracle
    from instance_stixels_amd import synthetic
    assign, load = reference_functions()
    need = dict(instance=200, labelled=50, rule=10, background=10, ties=5, group=1)
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
        C, S = secs.shape
        w = cols // C
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
        gt = np.clip(ir.synth_gt(inst, seed=seed + 40)[0], 0, 65535)
        patches(gt, secs, rows, cols, np.random.default_rng(seed + 41))
        assert gt.min() >= 0 and gt.max() <= 65535
        stixels = [[dict(vB=int(s["vB"]), vT=int(s["vT"]), type=int(s["type"]))
                    for s in secs[c, :rr.column_count(secs[c])]] for c in range(C)]
        for c in range(C):
            for i, s in enumerate(stixels[c]):
                s["class"] = int(secs[c, i]["semantic_class"])
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "x_gtFine_instanceIds.png")
            Image.fromarray(gt.astype(np.uint16)).save(path)
            assert np.array_equal(np.array(Image.open(path)), gt), "the 16-bit PNG does not round-trip"
            masks = load(path)
        labelled = assign(stixels, masks)
        ref_labels = np.full((C, S), -2, np.int32)   # -2: the reference gave the stixel no label (class < 11, no stixel)
        for c in range(C):
            for i, s in enumerate(labelled[c]):
                if "instance_label" in s:
                    ref_labels[c, i] = s["instance_label"]
        st = stats(stixels, masks, labelled, rows, w)
        print(f"case {k}: {preset} {rows}x{cols}x{D} (w = {w}, cols % 8 = {cols % 8}): {st}")
        for name, least in need.items():
            assert st[name] >= least, f"case {k}: {name} = {st[name]} < {least}: pick another seed"
        out[f"c{k}_sections"] = secs.view(np.int32).reshape(C, S, 8)
        out[f"c{k}_gt"] = gt.astype(np.uint16)
        out[f"c{k}_ref_labels"] = ref_labels
        out[f"c{k}_meta"] = np.array([rows, cols, D, seed, n_slabs], np.int32)
        out[f"c{k}_stats"] = np.array([st[n] for n in need], np.int32)
        out[f"c{k}_preset"] = np.frombuffer(preset.encode(), np.uint8)
    out["n_cases"] = np.array(len(CASES), np.int32)
    out["stat_names"] = np.frombuffer(",".join(need).encode(), np.uint8)
    np.savez_compressed(os.path.join(HERE, "assign_gt_reference_python.npz"), **out)
    print("written", os.path.join(HERE, "assign_gt_reference_python.npz"))


if __name__ == "__main__":
    main()
