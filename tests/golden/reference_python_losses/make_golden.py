"""Generates tests/golden/reference_python_losses/offset_losses_reference_python.npz -- the pin of f12 (is_offset_loss)
on the reference's own Python.

BUILD-CONTAINER ONLY: reads the reference checkout (REFERENCE, default: a checkout beside this repository) at
generation time; only the resulting vectors (data) are committed and travel to the GPU box.

What is executed from the reference, byte for byte as it stands there, cut out of the parsed source (ast) as
tests/golden/reference_python_targets/make_golden.py does: the classes DisparityOffsetLossSL and OffsetLossSL of
tools/CNN_training/losses.py, in a namespace that holds only `torch`.  That `torch` is a proxy whose one difference is
`Tensor(sequence)`: the reference packs the five values of `separate=True` with torch.Tensor(..), which is float32
whatever the inputs are; the proxy stacks them in the dtype of the run, so the float64 run keeps float64 terms.
For the same reason Tensor.float() means Tensor.double() while the float64 run lasts: the reference takes the cell
positions with `mask_ind.float()`, whose mean (1/3, say) would otherwise be rounded to float32 in the middle of a
binary64 evaluation.

Per case one frame per call, on the CPU, in float64 (THE DEFINITION, key "d") and in float32 (for the record, key "s"),
both abs_variance settings: DisparityOffsetLossSL with separate=True for the terms and without for the loss whose
torch.autograd.grad is the gradient; OffsetLossSL (which has no `separate` and swallows abs_variance) on the two
offset planes for the loss and the gradient.  The weights are exact in float32, the type the C ABI takes them in.

The generator REFUSES to write a fixture in which an argument of a sign lies in (0, 1e-4) in magnitude (rounding must
decide no sign), or one that lacks a corner case `stats` counts.

    python tests/golden/reference_python_losses/make_golden.py
"""
import ast
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get("REFERENCE", os.path.abspath(os.path.join(HERE, "..", "..", "..", "..", "reference")))
REF_LOSSES = os.path.join(REFERENCE, "tools/CNN_training/losses.py")
OUT = os.path.join(HERE, "offset_losses_reference_python.npz")
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import offset_loss_reference as lr  # noqa: E402

WEIGHTS = (2.0 ** -10, 2.0 ** -13, 2.0 ** -9, 2.0 ** -12)
GUARD = 1e-4


def reference_classes(dtype):
    import torch

    class Proxy(types.ModuleType):
        def __getattr__(self, name):
            return getattr(torch, name)

    proxy = Proxy("torch")
    proxy.Tensor = lambda values: torch.stack([torch.as_tensor(v, dtype=dtype).detach() for v in values])
    tree = ast.parse(open(REF_LOSSES).read())
    picked = [c for c in tree.body if isinstance(c, ast.ClassDef) and c.name in ("DisparityOffsetLossSL", "OffsetLossSL")]
    assert len(picked) == 2
    ns = {"torch": proxy}
    exec(compile(ast.Module(body=picked, type_ignores=[]), REF_LOSSES, "exec"), ns)
    return ns["DisparityOffsetLossSL"], ns["OffsetLossSL"]


def blobs(rng, ids, q, keys, most):
    Hs, Ws = ids.shape
    for key in keys:
        h, w = int(rng.integers(1, most)), int(rng.integers(1, most))
        y0, x0 = int(rng.integers(0, Hs - h + 1)), int(rng.integers(0, Ws - w + 1))
        yy, xx = np.mgrid[0:h, 0:w]
        blob = ((yy - (h - 1) / 2) / (h / 2)) ** 2 + ((xx - (w - 1) / 2) / (w / 2)) ** 2 <= 1.0
        ids[y0:y0 + h, x0:x0 + w][blob] = key
        q[y0:y0 + h, x0:x0 + w][blob] = int(rng.integers(1, 200)) + (yy[blob] % 3)


def frames(seed):
    """name -> (pred float32 [3][Hs][Ws], ids int32, d8 uint16)."""
    rng = np.random.default_rng(seed)
    out = {}

    def finish(name, ids, q, fixed=()):
        Hs, Ws = ids.shape
        pred = np.stack([rng.normal(40, 25, (Hs, Ws)), rng.normal(0, 3, (Hs, Ws)), rng.normal(0, 4, (Hs, Ws))])
        pred = pred.astype(np.float32)
        for (y, x), v in fixed:
            pred[:, y, x] = v
        d8 = (q.astype(np.int64) * 256 + rng.integers(0, 256, q.shape)).astype(np.uint16)
        d8[q == 0] = rng.integers(0, 256, int((q == 0).sum()))      # q == 0 whatever the low byte is
        out[name] = (pred, ids.astype(np.int32), d8)

    # the general frame: 24 x 50 cells (a wave straddles row ends), every id class and every exact zero
    Hs, Ws = 24, 50
    pool = np.array([7, 8, 10, 11, 21, 255, 1000, -1, -5, 0, 33], np.int32)
    ids = pool[rng.integers(0, pool.size, (Hs // 4, Ws // 5))].repeat(4, 0).repeat(5, 1)
    q = rng.integers(0, 3, ids.shape) * 20
    blobs(rng, ids, q, [26001, 26002, 24001, 1001, 33005, 25007, 28001, 26003], 12)
    q[rng.random(q.shape) < 0.2] = 0
    fixed = []
    for k, v in enumerate((10, 11, 255, 1000, 1001, -7)):
        ids[0, k] = v
    ids[1, 0] = 7; fixed.append(((1, 0), (0.0, 0.0, 0.0)))                  # a stuff cell with a 0 prediction
    ids[2, 0] = 32042; q[2, 0] = 9; fixed.append(((2, 0), (9.0, 0.0, 0.0)))   # n = 1: pos == g, disp == med
    ids[3, 0:2] = 32043; q[3, 0:2] = (5, 0)                                 # n = 2
    ids[4, 0:3] = 32044; q[4, 0:3] = 0                                      # n = 3, no non-zero q, all pos equal
    for x in range(3):
        fixed.append(((4, x), (12.5, 2.0, 10.0 - x)))
    for (y, x) in ((6, 0), (6, 1), (Hs - 1, Ws - 1), (Hs - 2, Ws - 1)):     # one key in two parts
        ids[y, x] = 27011; q[y, x] = 30
    for x, v in ((0, 43), (1, 79), (2, 0)):                                 # an even count, middle values 43 and 79
        ids[8, x] = 25090; q[8, x] = v
    for x, v in ((0, 40), (1, 10), (2, 30), (3, 20)):                       # the lower median of 10 20 30 40 is 20
        ids[9, x] = 25091; q[9, x] = v
    fixed.append(((9, 0), (20.0, 1.5, -2.25)))                              # disp == med in a larger key
    finish("general", ids, q, fixed)

    # no key at all
    ids = np.array([7, 11, 255, 1000, 300, -3], np.int32)[rng.integers(0, 6, (16, 32))]
    finish("no_keys", ids, rng.integers(0, 100, ids.shape))

    # no stuff: nan terms, a finite gradient
    ids = np.array([11, 21, 1000, 300], np.int32)[rng.integers(0, 4, (5, 7))]
    q = rng.integers(0, 100, ids.shape)
    blobs(rng, ids, q, [26001, 24002, 1001], 4)
    finish("no_stuff", ids, q)

    # 70 keys in 16 x 32 cells
    ids = np.full((16, 32), 8, np.int32)
    ids[:, 20:] = 21
    q = rng.integers(0, 4, ids.shape) * 33
    for k in range(70):
        y, x = divmod(k, 10)
        ids[2 * y:2 * y + 1 + k % 2, 3 * x:3 * x + 1 + k % 3] = 24000 + 37 * k % 9000 + 1001
    finish("many_keys", ids, q)

    # a few cells
    ids = np.array([[26001, 7, 26001], [11, 26001, 255]], np.int32)
    finish("tiny", ids, np.array([[4, 0, 9], [1, 0, 2]]))
    return out


def stats(cases):
    """The corner cases, counted over all frames from the restatement's sign arguments and the inputs."""
    k = dict(zero_stuff=0, zero_pos_g=0, zero_disp_med=0, equal_pos=0, n1=0, n2=0, n3=0, id10=0, id11=0, id255=0,
             id1000=0, id1001=0, negative_id=0, two_parts=0, no_disparity=0, even_median=0, no_keys=0, no_stuff=0,
             keys65=0)
    for pred, ids, d8 in cases.values():
        args = {}
        lr.frame(pred, ids, d8, WEIGHTS, True, sign_args=args)
        k["zero_stuff"] += int((np.array(args.get("stuff_off", [1])) == 0).sum() > 0
                               and (np.array(args.get("stuff_disp", [1])) == 0).sum() > 0)
        k["zero_pos_g"] += int((np.array(args.get("pos_g", [1])) == 0).sum())
        k["zero_disp_med"] += int((np.array(args.get("disp_med", [1])) == 0).sum())
        for v in (10, 11, 255, 1000, 1001):
            k[f"id{v}"] += int((ids == v).sum())
        k["negative_id"] += int((ids < 0).sum())
        keys = np.unique(ids[ids > 1000]).tolist()
        k["no_keys"] += not keys
        k["keys65"] += len(keys) >= 65
        k["no_stuff"] += not ((ids < 11) | (ids == 255)).any()
        q = d8.astype(np.int64) >> 8
        for key in keys:
            ys, xs = np.nonzero(ids == key)
            n = ys.size
            k["n1"] += n == 1; k["n2"] += n == 2; k["n3"] += n == 3
            pos = pred[1:, ys, xs].astype(np.float64) + np.stack([ys, xs])
            k["equal_pos"] += n > 2 and bool((pos == pos[:, :1]).all())
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
            qs = np.sort(q[ys, xs][q[ys, xs] != 0])
            k["no_disparity"] += qs.size == 0
            k["even_median"] += qs.size > 0 and qs.size % 2 == 0 and qs[qs.size // 2 - 1] != qs[qs.size // 2]
    return {a: int(b) for a, b in k.items()}


def guarded(cases):
    """No argument of a sign in (0, GUARD), in either abs_variance setting."""
    for name, (pred, ids, d8) in cases.items():
        for abs_variance in (False, True):
            args = {}
            lr.frame(pred, ids, d8, WEIGHTS, abs_variance, sign_args=args)
            for kind, values in args.items():
                v = np.abs(np.array(values))
                if ((v > 0) & (v < GUARD)).any():
                    return f"{name}: {kind} has {v[(v > 0) & (v < GUARD)].min()}"
    return None


def run_reference(pred, ids, d8, dtype):
    """The reference on one frame -> dict of float64 arrays."""
    import torch
    D, O = reference_classes(dtype)
    w = dict(offset_mean_weight=WEIGHTS[0], offset_variance_weight=WEIGHTS[1], disparity_mean_weight=WEIGHTS[2],
             disparity_variance_weight=WEIGHTS[3])
    gt = torch.from_numpy(ids.astype(np.int64))[None]
    disp = torch.from_numpy((d8.astype(np.int64) >> 8).astype(np.float64)).to(dtype)[None]
    out = {}
    keep = torch.Tensor.float
    if dtype == torch.float64:
        torch.Tensor.float = lambda t, *a, **k: t.double()
    try:
        _run(out, D, O, w, pred, gt, disp, dtype)
    finally:
        torch.Tensor.float = keep
    return out


def _run(out, D, O, w, pred, gt, disp, dtype):
    import torch
    for a in (0, 1):
        p = torch.from_numpy(pred.astype(np.float64)).to(dtype)[None].requires_grad_(True)
        fn = D(abs_variance=bool(a), **w)
        out[f"D{a}_five"] = fn(p, gt, disp, separate=True).detach().numpy().astype(np.float64)
        loss = fn(p, gt, disp)
        out[f"D{a}_loss"] = np.float64(loss.item())
        out[f"D{a}_grad"] = torch.autograd.grad(loss, p)[0][0].numpy().astype(np.float64)
        p2 = torch.from_numpy(pred[1:].astype(np.float64)).to(dtype)[None].requires_grad_(True)
        loss = O(abs_variance=bool(a), **w)(p2, gt)
        out[f"O{a}_loss"] = np.float64(loss.item())
        out[f"O{a}_grad"] = torch.autograd.grad(loss, p2)[0][0].numpy().astype(np.float64)


def main():
    import torch
    for seed in range(1, 200):
        cases = frames(seed)
        why = guarded(cases)
        if why is None:
            break
        print(f"seed {seed}: {why}")
    else:
        raise SystemExit("no seed passes the sign guard")
    st = stats(cases)
    print(f"seed {seed}: {st}")
    for name, have in st.items():
        assert have >= 1, f"no {name}: change the frames"
    out = {"names": np.frombuffer(",".join(cases).encode(), np.uint8), "weights": np.array(WEIGHTS, np.float64),
           "stat_names": np.frombuffer(",".join(st).encode(), np.uint8), "stats": np.array(list(st.values()), np.int32),
           "seed": np.array(seed, np.int32), "guard": np.array(GUARD)}
    for name, (pred, ids, d8) in cases.items():
        out[f"{name}_pred"], out[f"{name}_ids"], out[f"{name}_d8"] = pred, ids, d8
        for tag, dtype in (("d", torch.float64), ("s", torch.float32)):
            for key, value in run_reference(pred, ids, d8, dtype).items():
                out[f"{name}_{tag}_{key}"] = value
        five = out[f"{name}_d_D0_five"]
        print(f"{name}: {pred.shape[1]}x{pred.shape[2]} float64 five {five} grad finite "
              f"{bool(np.isfinite(out[f'{name}_d_D0_grad']).all())}")
    np.savez_compressed(OUT, **out)
    print("written", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
