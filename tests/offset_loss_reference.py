"""A numpy restatement of f12 (is_offset_loss of include/instance_stixels_core.h): the reference's OffsetLossSL and
DisparityOffsetLossSL (tools/CNN_training/losses.py) in float64 on the float32 inputs, with the gradient in closed
form.  It is pinned on the reference's own classes (float64 run, torch.autograd.grad) by tests/test_offset_loss.py
through tests/golden/reference_python_losses.  `torch_loop_loss` is a torch loop of the reference's structure (unique,
nonzero, gather, var, median per instance id, autograd backwards): the timing yardstick where the reference itself
does not exist."""
import numpy as np

TERMS = ("offset_mean", "offset_variance", "disparity_mean", "disparity_variance")


def lower_median(values):
    """torch.median of a 1-d array: the lower of the middle pair."""
    s = np.sort(np.asarray(values))
    return s[(s.size - 1) // 2]


def frame(pred, ids, d8=None, weights=(1e-3, 1e-4, 1e-3, 1e-4), abs_variance=False, sign_args=None):
    """One frame.  pred float32 [planes][Hs][Ws] (planes 2: off_y, off_x; 3: disp, off_y, off_x), ids int [Hs][Ws],
    d8 uint16 [Hs][Ws] raw disparity at 1/8 (3 planes).  Returns (terms float64 [4], grad float64 [planes][Hs][Ws]);
    the gradient is that of sum(weights * terms).  sign_args: a dict that receives every argument of a sign, by kind
    (pos_g, pos_m, disp_md, disp_med, stuff_off, stuff_disp)."""
    pred = np.asarray(pred)
    assert pred.dtype == np.float32 and pred.ndim == 3 and pred.shape[0] in (2, 3)
    planes, Hs, Ws = pred.shape
    P = pred.astype(np.float64)
    ids = np.asarray(ids).astype(np.int64)
    w_om, w_ov, w_dm, w_dv = [float(w) for w in weights]
    if planes == 2:
        w_dm = w_dv = 0.0
    off = P[-2:]
    disp = P[0] if planes == 3 else None
    q = (np.asarray(d8).astype(np.int64) >> 8) if planes == 3 else None
    terms = np.zeros(4, np.float64)
    grad = np.zeros_like(P)
    goff = grad[-2:]

    def note(kind, values):
        if sign_args is not None:
            sign_args.setdefault(kind, []).extend(values)

    def add(target, where, weight, value):
        if weight != 0.0:        # a zero weight removes the line (and keeps 0 * nan out of the gradient)
            target[where] += weight * value

    for key in np.unique(ids[ids > 1000]).tolist():
        ys, xs = np.nonzero(ids == key)
        n = ys.size
        cell = np.stack([ys, xs]).astype(np.float64)
        pos = off[:, ys, xs] + cell
        g = cell.sum(axis=1, keepdims=True) / n
        m = pos.sum(axis=1, keepdims=True) / n
        terms[0] += np.abs(pos - g).sum() / n / 2
        note("pos_g", (pos - g).ravel().tolist())
        for ax in range(2):
            add(goff[ax], (ys, xs), w_om, np.sign(pos[ax] - g[ax]) / (2 * n))
        if not abs_variance:
            terms[1] += (((pos - m) ** 2).sum(axis=1) / n).sum() / 2
            for ax in range(2):
                add(goff[ax], (ys, xs), w_ov, (pos[ax] - m[ax]) / n)
        elif n > 2:
            terms[1] += np.abs(pos - m).sum() / n / 2
            note("pos_m", (pos - m).ravel().tolist())
            for ax in range(2):
                s = np.sign(pos[ax] - m[ax])
                add(goff[ax], (ys, xs), w_ov, (s - s.sum() / n) / (2 * n))
        if planes == 3:
            dk = disp[ys, xs]
            md = dk.sum() / n
            if not abs_variance:
                terms[3] += ((dk - md) ** 2).sum() / n
                add(grad[0], (ys, xs), w_dv, 2 * (dk - md) / n)
            elif n > 2:
                terms[3] += np.abs(dk - md).sum() / n
                note("disp_md", (dk - md).tolist())
                s = np.sign(dk - md)
                add(grad[0], (ys, xs), w_dv, (s - s.sum() / n) / n)
            qk = q[ys, xs]
            qk = qk[qk != 0]
            if qk.size:
                med = float(lower_median(qk))
                terms[2] += np.abs(dk - med).sum() / n
                note("disp_med", (dk - med).tolist())
                add(grad[0], (ys, xs), w_dm, np.sign(dk - med) / n)
    stuff = (ids < 11) | (ids == 255)
    s = int(stuff.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        terms[0] += np.float64(np.abs(off[:, stuff]).sum()) / np.float64(s) / 2     # 0 / 0 without stuff, as the reference
        if planes == 3:
            terms[2] += np.float64(np.abs(disp[stuff]).sum()) / np.float64(s)
    note("stuff_off", off[:, stuff].ravel().tolist())
    if s:
        for ax in range(2):
            add(goff[ax], stuff, w_om, np.sign(off[ax][stuff]) / (2 * s))
        if planes == 3:
            note("stuff_disp", disp[stuff].tolist())
            add(grad[0], stuff, w_dm, np.sign(disp[stuff]) / s)
    return terms, grad


def batch(pred, ids, d8=None, weights=(1e-3, 1e-4, 1e-3, 1e-4), abs_variance=False):
    """The call of the C ABI in float64: (loss5 [5], terms [n][4], grad [n][planes][Hs][Ws])."""
    pred = np.asarray(pred)
    n, planes = pred.shape[:2]
    terms = np.zeros((n, 4), np.float64)
    grad = np.zeros(pred.shape, np.float64)
    for f in range(n):
        terms[f], grad[f] = frame(pred[f], ids[f], d8[f] if d8 is not None else None, weights, abs_variance)
    sums = np.zeros(4, np.float64)
    for f in range(n):      # ascending, as the reference's +=
        sums = sums + terms[f]
    w = [float(v) for v in weights]
    loss = w[0] * sums[0] + w[1] * sums[1]
    if planes == 3:
        loss = loss + w[2] * sums[2] + w[3] * sums[3]
    return np.concatenate([[loss], sums]), terms, grad


def key_counts(ids):
    return np.array([np.unique(f[f > 1000]).size for f in np.asarray(ids)], np.int32)


def ulp_distance(got, want64):
    """|got - fl32(want)| in units of the float32 ulp at want, elementwise; 0 where both are NaN (inf where one is)."""
    got = np.asarray(got, np.float32).astype(np.float64)
    want64 = np.asarray(want64, np.float64)
    want32 = want64.astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        ulp = np.spacing(np.abs(want32)).astype(np.float64)
        dist = np.abs(got - want64) / ulp
    both_nan = np.isnan(got) & np.isnan(want64)
    one_nan = np.isnan(got) ^ np.isnan(want64)
    dist = np.where(both_nan, 0.0, dist)
    dist = np.where(one_nan, np.inf, dist)
    return np.where((want64 == 0) & (got != 0), np.inf, dist)      # an exact zero must be exact


def torch_loop_loss(prediction, instance_gt, disparity_q=None, weights=(1e-3, 1e-4, 1e-3, 1e-4), abs_variance=False):
    """The loop of the reference's two classes restated on torch tensors of any device and float dtype: prediction
    [n][planes][Hs][Ws] (requires_grad for a backward), instance_gt [n][Hs][Ws] integer, disparity_q [n][Hs][Ws]
    integral q = raw // 256 (3 planes).  Returns (loss, the four sums) as tensors."""
    import torch
    planes = prediction.shape[1]
    om = ov = dm = dv = 0
    for f in range(prediction.shape[0]):
        gt, pred = instance_gt[f], prediction[f]
        ids = torch.unique(gt)
        for key in ids[ids > 1000]:
            ind = torch.nonzero(gt == key).t()
            n = ind.size(1)
            cell = ind.to(pred.dtype)
            pos = pred[-2:, ind[0], ind[1]] + cell
            g = cell.mean(dim=1).reshape(2, 1).detach()
            om = om + (pos - g).abs().sum() / n / 2
            if not abs_variance:
                ov = ov + pos.var(dim=1, unbiased=False).sum() / 2
            elif n > 2:
                ov = ov + (pos - pos.mean(dim=1).reshape(2, 1)).abs().sum() / n / 2
            if planes == 3:
                dk = pred[0, ind[0], ind[1]]
                qk = disparity_q[f][ind[0], ind[1]]
                qk = qk[qk != 0]
                if not abs_variance:
                    dv = dv + dk.var(unbiased=False)
                elif n > 2:
                    dv = dv + (dk - dk.mean()).abs().sum() / n
                if len(qk) > 0:
                    dm = dm + (dk - qk.median()).abs().sum() / n
        stuff = (gt < 11) | (gt == 255)
        s = stuff.sum()
        om = om + pred[-2:, stuff].abs().sum() / s / 2
        if planes == 3:
            dm = dm + pred[0, stuff].abs().sum() / s
    w = [float(v) for v in weights]
    loss = w[0] * om + w[1] * ov
    if planes == 3:
        loss = loss + w[2] * dm + w[3] * dv
    return loss, (om, ov, dm, dv)
