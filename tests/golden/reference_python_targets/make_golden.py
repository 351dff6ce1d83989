"""Generates tests/golden/reference_python_targets/gt_targets_reference_python.npz -- the pin of f11
(is_mode_downsample / is_gt_instance_targets / Stixels::GroundTruthOffsetsBatch) on the reference's own Python.

BUILD-CONTAINER ONLY: reads the reference checkout (REFERENCE, default /root/reference) at generation time; only
the resulting vectors (data) are committed and travel to the GPU box.

What is executed from the reference, byte for byte as it stands there, cut out of the parsed sources (ast) as
tests/golden/reference_python_gt/make_golden.py does:
  modefilter_np                 tools/CNN_training/datasets/transforms.py:59-70   (a method of ModeDownsample)
  _instance_offsets             tools/CNN_training/datasets/cityscapes.py:146-167 (a method of the data set)
  _instance_offsets_disparity   tools/CNN_training/datasets/cityscapes.py:114-144
each in a namespace that holds ONLY what it needs (numpy for the first, torch for the others) and called with
self = None.  The disparity goes in as a float32 tensor of integral values: with an integer tensor the installed torch
refuses the reference's index assignment of a float median, and `//` is the same floor division either way.

Per case (small frames, CPU only): a hand-built instanceIds image and raw uint16 disparity -> modefilter_np of both ->
the two target functions on the downsampled images.  The generator REFUSES to write a fixture that lacks one of the
corner cases `stats` counts.

    python tests/golden/reference_python_targets/make_golden.py
"""
import ast
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get("REFERENCE", "/root/reference")
REF_TRANSFORMS = os.path.join(REFERENCE, "tools/CNN_training/datasets/transforms.py")
REF_DATASET = os.path.join(REFERENCE, "tools/CNN_training/datasets/cityscapes.py")
OUT = os.path.join(HERE, "gt_targets_reference_python.npz")

CASES = [(64, 128, 1), (96, 200, 2), (128, 256, 3)]   # rows, cols, seed


def _cut_method(path, name, ns):
    tree = ast.parse(open(path).read())
    picked = [f for c in tree.body if isinstance(c, ast.ClassDef) for f in c.body
              if isinstance(f, ast.FunctionDef) and f.name == name]
    assert len(picked) == 1, name
    exec(compile(ast.Module(body=picked, type_ignores=[]), path, "exec"), ns)
    return ns[name]


def reference_functions():
    import torch
    mode = _cut_method(REF_TRANSFORMS, "modefilter_np", {"np": np})
    off2 = _cut_method(REF_DATASET, "_instance_offsets", {"torch": torch})
    off3 = _cut_method(REF_DATASET, "_instance_offsets_disparity", {"torch": torch})
    return mode, off2, off3


def frame(rows, cols, seed):
    """An instanceIds image and a raw disparity with the corner cases at fixed cells (8x8 blocks), the rest a random
    Cityscapes-like scene whose instance borders do not follow the blocks."""
    rng = np.random.default_rng(seed)
    Hs, Ws = rows // 8, cols // 8
    stuff = np.array([7, 8, 11, 21, 23], np.int32)
    gt = stuff[rng.integers(0, stuff.size, (Hs // 2 + 1, Ws // 4 + 1))].repeat(16, 0).repeat(32, 1)[:rows, :cols].copy()
    disp = np.zeros((rows, cols), np.int64)
    labs = [24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 13]     # caravan, trailer and a trainId-style label too
    for k in range(10 + 2 * seed):
        h, w = int(rng.integers(5, rows // 3)), int(rng.integers(5, cols // 4))
        y0, x0 = int(rng.integers(0, rows - h)), int(rng.integers(0, cols - w))
        yy, xx = np.mgrid[0:h, 0:w]
        blob = ((yy - h / 2) / (h / 2)) ** 2 + ((xx - w / 2) / (w / 2)) ** 2 <= 1.0
        gt[y0:y0 + h, x0:x0 + w][blob] = labs[k % len(labs)] * 1000 + k // len(labs) + (k % 3 == 0)
        q = int(rng.integers(1, 120))
        patch = disp[y0:y0 + h, x0:x0 + w]
        patch[blob] = (q + (yy[blob] // 6) % 3) * 256 + 128
        patch[blob & ((yy + xx) % 5 == 0)] = 0              # holes
    disp[disp == 0] = np.where(rng.random(int((disp == 0).sum())) < 0.5, 0, 20 * 256 + 7)

    def cell(y, x):
        return gt[8 * y:8 * y + 8, 8 * x:8 * x + 8], disp[8 * y:8 * y + 8, 8 * x:8 * x + 8]

    # a two-way tie: the smaller value wins, once an instance id against a larger one, once stuff against an id
    g, _ = cell(0, 0); g[:, :4] = 26007; g[:, 4:] = 26003
    g, _ = cell(0, 1); g[:4] = 26003; g[4:] = 23
    # a three-way tie, 21 : 21 : 21 and one pixel of a fourth value
    g, _ = cell(0, 2); g[...] = np.array([33001] * 21 + [26003] * 21 + [28002] * 21 + [5], np.int32).reshape(8, 8)
    # a value <= 1000 beats an instance id
    g, _ = cell(0, 3); g[...] = 7; g[:3] = 26003
    # ids 1000 and 1001
    g, _ = cell(1, 0); g[...] = 1000
    g, _ = cell(1, 1); g[...] = 1001
    # one instance in two disconnected parts
    for (y, x) in ((2, 0), (2, 1), (Hs - 1, Ws - 1), (Hs - 2, Ws - 1), (Hs - 1, Ws - 2)):
        g, _ = cell(y, x); g[...] = 27011
    # a one-cell instance
    g, _ = cell(3, 0); g[...] = 32042
    # n = 3 with sums divisible by 3: cells (4, 3), (4, 4), (4, 5)
    for x in (3, 4, 5):
        g, d = cell(4, x); g[...] = 24077; d[...] = 0    # ... and it has no non-zero disparity
    # an even count of non-zero q whose two middle values differ: 43 and 79 (and one zero)
    for x, q in ((7, 43), (8, 79), (9, 0)):
        g, d = cell(5, x); g[...] = 25090; d[...] = q * 256 + (3 if q else 0)
    # four non-zero values 10, 20, 30, 40: the lower median is 20
    for x, q in ((7, 40), (8, 10), (9, 30), (10, 20)):
        g, d = cell(6, x); g[...] = 25091; d[...] = q * 256 + 255
    return gt.astype(np.int32), disp.astype(np.uint16)


def stats(gt, ids8, d8, off2):
    """The corner cases, counted from the images and the reference's answers."""
    Hs, Ws = ids8.shape
    k = dict(tie2=0, tie3=0, stuff_beats_id=0, id1000=0, id1001=0, two_parts=0, one_cell=0, n3_integer=0,
             negative_fraction=0, even_median=0, no_disparity=0)
    for y in range(Hs):
        for x in range(Ws):
            vals, cnt = np.unique(gt[8 * y:8 * y + 8, 8 * x:8 * x + 8], return_counts=True)
            top = int((cnt == cnt.max()).sum())
            k["tie2"] += top == 2
            k["tie3"] += top >= 3
            k["stuff_beats_id"] += ids8[y, x] <= 1000 and bool((vals > 1000).any())
    k["id1000"] = int((ids8 == 1000).sum())
    k["id1001"] = int((ids8 == 1001).sum())
    q8 = d8.astype(np.int64) // 256
    for key in np.unique(ids8[ids8 > 1000]).tolist():
        m = ids8 == key
        ys, xs = np.nonzero(m)
        n = ys.size
        k["one_cell"] += n == 1
        k["n3_integer"] += (n & (n - 1)) != 0 and (8 * ys.sum()) % n == 0 and (8 * xs.sum()) % n == 0
        # disconnected: a flood fill over 4-neighbours from the first cell does not reach every cell
        seen = {(int(ys[0]), int(xs[0]))}
        todo = list(seen)
        cells = set(zip(ys.tolist(), xs.tolist()))
        while todo:
            cy, cx = todo.pop()
            for nb in ((cy + 1, cx), (cy - 1, cx), (cy, cx + 1), (cy, cx - 1)):
                if nb in cells and nb not in seen:
                    seen.add(nb)
                    todo.append(nb)
        k["two_parts"] += len(seen) < n
        qs = np.sort(q8[m][q8[m] != 0])
        k["no_disparity"] += qs.size == 0
        k["even_median"] += qs.size > 0 and qs.size % 2 == 0 and qs[qs.size // 2 - 1] != qs[qs.size // 2]
    e = np.float32(8.0) * off2
    k["negative_fraction"] = int(((e < 0) & (e != np.trunc(e))).sum())
    return k


def main():
    import torch
    mode, off2_fn, off3_fn = reference_functions()
    out = {}
    names = None
    for c, (rows, cols, seed) in enumerate(CASES):
        gt, disp = frame(rows, cols, seed)
        ids8 = mode(None, gt, 8)
        d8 = mode(None, disp, 8)
        assert ids8.dtype == np.int32 and d8.dtype == np.uint16
        off2 = off2_fn(None, torch.from_numpy(ids8.copy())).numpy()
        off3 = off3_fn(None, torch.from_numpy(ids8.copy()), torch.from_numpy(d8.astype(np.float32))).numpy()
        assert off2.dtype == np.float32 and off3.dtype == np.float32
        assert np.array_equal(off2.view(np.uint32), off3[1:].view(np.uint32)), "the reference's two functions disagree"
        st = stats(gt, ids8, d8, off2)
        print(f"case {c}: {rows}x{cols}: {st}")
        for name, have in st.items():
            assert have >= 1, f"case {c}: no {name}: change the frame"
        names = list(st)
        out[f"c{c}_gt"] = gt.astype(np.uint16)
        out[f"c{c}_disparity"] = disp
        out[f"c{c}_ids8"] = ids8.astype(np.uint16)
        out[f"c{c}_disparity8"] = d8
        out[f"c{c}_targets3"] = off3
        out[f"c{c}_stats"] = np.array([st[n] for n in names], np.int32)
        assert gt.min() >= 0 and gt.max() <= 65535
    out["n_cases"] = np.array(len(CASES), np.int32)
    out["stat_names"] = np.frombuffer(",".join(names).encode(), np.uint8)
    np.savez_compressed(OUT, **out)
    print("written", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
