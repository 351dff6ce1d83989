"""The reference of the head's backward pass and of the semantic NLL loss (instance_stixels_core.h f14), independent
of the kernels.  The two fp32 chains of the contract (dX over the channels, the chunk partials of dW / db over the
pixels) and the binary64 reduction of the partials are short C functions compiled with the host compiler on first use,
as tests/head_reference.py does (-ffp-contract=off; fmaf is the correctly rounded fused operation); dz, the loss and
every tolerance are numpy float64."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

SOURCE = r"""
#include <math.h>
#include <stddef.h>
/* w [C][K], dz [C][P] -> dx [K][P]: one fp32 chain per (k, p) in increasing c, from +0 */
void head_dx(const float* w, const float* dz, float* dx, int C, int K, long P) {
    for (int k = 0; k < K; k++)
        for (long p = 0; p < P; p++) {
            float acc = 0.0f;
            for (int c = 0; c < C; c++) acc = fmaf(w[(size_t)c * K + k], dz[(size_t)c * P + p], acc);
            dx[(size_t)k * P + p] = acc;
        }
}
/* dz [C][P], x [K][P] -> part [chunks][C][K + 1]: per chunk of T pixels one fp32 chain per (c, k) in increasing p,
 * from +0; column K is the plain fp32 sum of dz */
void head_partials(const float* dz, const float* x, float* part, int C, int K, long P, long T) {
    long chunks = (P + T - 1) / T;
    for (long j = 0; j < chunks; j++) {
        long end = (j + 1) * T < P ? (j + 1) * T : P;
        for (int c = 0; c < C; c++) {
            float* out = part + ((size_t)j * C + c) * (K + 1);
            for (int k = 0; k < K; k++) {
                float acc = 0.0f;
                for (long p = j * T; p < end; p++) acc = fmaf(dz[(size_t)c * P + p], x[(size_t)k * P + p], acc);
                out[k] = acc;
            }
            float acc = 0.0f;
            for (long p = j * T; p < end; p++) acc = acc + dz[(size_t)c * P + p];
            out[K] = acc;
        }
    }
}
/* part [parts][m] -> out [m]: binary64 sums in increasing part, rounded once */
void head_reduce(const float* part, float* out, long parts, long m) {
    for (long i = 0; i < m; i++) {
        double s = 0.0;
        for (long w = 0; w < parts; w++) s += (double)part[(size_t)w * m + i];
        out[i] = (float)s;
    }
}
"""
_LIB = None
_DIR = None


def _lib():
    global _LIB, _DIR
    if _LIB is None:
        _DIR = tempfile.TemporaryDirectory(prefix="head_backward_reference_")
        src, so = os.path.join(_DIR.name, "head_backward.c"), os.path.join(_DIR.name, "libhead_backward.so")
        with open(src, "w") as f:
            f.write(SOURCE)
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", src, "-o", so, "-lm"],
                       check=True)
        _LIB = ctypes.CDLL(so)
        fp, ci, cl = ctypes.POINTER(ctypes.c_float), ctypes.c_int, ctypes.c_long
        _LIB.head_dx.argtypes = [fp, fp, fp, ci, ci, cl]
        _LIB.head_partials.argtypes = [fp, fp, fp, ci, ci, cl, cl]
        _LIB.head_reduce.argtypes = [fp, fp, cl, cl]
        for f in (_LIB.head_dx, _LIB.head_partials, _LIB.head_reduce):
            f.restype = None
    return _LIB


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def grad_features(weight, dz):
    """weight [C][K], dz [n][C][Hs][Ws] fp32 -> fp32 dX [n][K][Hs][Ws]: the contract's chain over the channels."""
    w = np.ascontiguousarray(weight, np.float32)
    d = np.ascontiguousarray(dz, np.float32)
    n, C, Hs, Ws = d.shape
    K = w.shape[1]
    assert w.shape == (C, K)
    dx = np.empty((n, K, Hs, Ws), np.float32)
    for i in range(n):
        _lib().head_dx(_fp(w), _fp(d[i]), _fp(dx[i]), C, K, Hs * Ws)
    return dx


def grad_weight_bias(features, dz, chunk):
    """features [n][K][Hs][Ws] (widened to fp32, exact for halves), dz [n][C][Hs][Ws] fp32 -> (dW [C][K], db [C]) fp32:
    the chunk partials of every frame, then their binary64 sums, frame outer and chunk inner."""
    x = np.ascontiguousarray(features, np.float32)
    d = np.ascontiguousarray(dz, np.float32)
    n, C, Hs, Ws = d.shape
    K, P = x.shape[1], Hs * Ws
    chunks = (P + chunk - 1) // chunk
    part = np.empty((n, chunks, C, K + 1), np.float32)
    for i in range(n):
        _lib().head_partials(_fp(d[i]), _fp(x[i]), _fp(part[i]), C, K, P, chunk)
    out = np.empty((C, K + 1), np.float32)
    _lib().head_reduce(_fp(part), _fp(out), n * chunks, C * (K + 1))
    return out[:, :K].copy(), out[:, K].copy()


def class_sum64(gy, n_classes):
    """S [n][1][Hs][Ws] float64: the class planes of gy added in increasing c."""
    S = np.zeros(gy[:, :1].shape, np.float64)
    for c in range(n_classes):
        S = S + gy[:, c:c + 1].astype(np.float64)
    return S


def dz64(y, gy, n_classes):
    """float64 [n][C][Hs][Ws]: exp(-y) S - gy on the class channels, gy on the others (exactly fp32 there)."""
    out = gy.astype(np.float64)
    S = class_sum64(gy, n_classes)
    out[:, :n_classes] = np.exp(-y[:, :n_classes].astype(np.float64)) * S - gy[:, :n_classes].astype(np.float64)
    return out


def dz(y, gy, n_classes):
    """fp32 [n][C][Hs][Ws]: dz64 rounded once (the regression channels are gy's bits)."""
    out = dz64(y, gy, n_classes).astype(np.float32)
    out[:, n_classes:] = gy[:, n_classes:]
    return out


def dz_tolerance(y, gy, n_classes):
    """The bound of the class channels of dz, float64 [n][n_classes][Hs][Ws]: ulp_fp32(want) + 2^-40 (|S| p + |gy|),
    the final rounding and a floor for binary64 exp implementations that differ in the last places."""
    want = dz64(y, gy, n_classes)[:, :n_classes]
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    p = np.exp(-y[:, :n_classes].astype(np.float64))
    return ulp + 2.0 ** -40 * (np.abs(class_sum64(gy, n_classes)) * p + np.abs(gy[:, :n_classes].astype(np.float64)))


def nll64(y, target, n_classes, ignore_index=255):
    """(loss float64, V, bad, unit gradient fp32 [n][n_classes][Hs][Ws]) of y [n][C][Hs][Ws] fp32 and integer targets
    [n][Hs][Ws]: loss = sum_valid y[t_p](p) / V (math.fsum: the correctly rounded sum, which any summation order of
    the device stays within a few binary64 ulps of), NaN with V = 0; a target outside [0, n_classes) that is not
    ignore_index is ignored and counted."""
    import math
    t = np.asarray(target).astype(np.int64)
    cls = (t >= 0) & (t < n_classes) & (t != ignore_index)
    bad = int((~cls & (t != ignore_index)).sum())
    V = int(cls.sum())
    picked = np.take_along_axis(y[:, :n_classes].astype(np.float64), np.where(cls, t, 0)[:, None], axis=1)[:, 0]
    loss = math.fsum(picked[cls].tolist()) / V if V else float("nan")
    grad = np.zeros((y.shape[0], n_classes) + y.shape[2:], np.float32)
    if V:
        unit = np.float32(1.0 / V)
        grad = np.where(cls[:, None] & (np.arange(n_classes)[None, :, None, None] == t[:, None]), unit,
                        np.float32(0)).astype(np.float32)
    return loss, V, bad, grad


def autograd_bounds(x, w, z_mag, y, gy, dzv, n_classes, chunk):
    """Bounds of |reference (or device) gradient - float64 autograd gradient| for (dX, dW, db), each in the
    gradient's shape, float64.  u = 2^-24 bounds the relative error of one fp32 rounding.

    Inputs of the error: the fp32 logits differ from the float64 ones by ez <= K u sum_k |w x| = K u z_mag (the chain
    bound of tests/test_segmentation_head_cpu.py); y = lse - z then differs by ey <= 2 max_c ez + 2 u |y| + 2^-40 (1 +
    |y|) (both logit errors, the rounding of y to fp32 with one more ulp for the device's binary64 log / exp, and
    their floor); p = exp(-y) by p expm1(ey); gy = (float)(1 / V) by u |gy| and S by u sum_c |gy|.  Hence
      e_dz[class j] = |S| p expm1(ey) + u (p sum_c |gy| + |gy_j| + |dz_j|), e_dz[regression] = u |gy| (the float64
      upstream gradient rounded to fp32), and
      dX:  sum_c |w| e_dz + CH u sum_c |w dz|                      (CH roundings, each below u sum |terms|)
      dW:  sum_p |x| e_dz + (min(T, P) + 1) u sum_p |dz x|         (a chain per chunk, then one rounding of the sum)
      db:  sum_p e_dz + (min(T, P) + 1) u sum_p |dz|
    all times 1.01 for the terms of second order."""
    u = 2.0 ** -24
    x64, w64 = np.abs(x.astype(np.float64)), np.abs(w.astype(np.float64))
    n, K, Hs, Ws = x.shape
    CH = w.shape[0]
    y64, gy64, d64 = y.astype(np.float64), np.abs(gy.astype(np.float64)), np.abs(dzv.astype(np.float64))
    ez = K * u * z_mag[:, :n_classes]
    ey = 2.0 * ez.max(axis=1, keepdims=True) + 2.0 * u * np.abs(y64[:, :n_classes]) + \
        2.0 ** -40 * (1.0 + np.abs(y64[:, :n_classes]))
    p = np.exp(-y64[:, :n_classes])
    S = np.abs(class_sum64(gy, n_classes))
    e_dz = u * gy64
    e_dz[:, :n_classes] = S * p * np.expm1(ey) + u * (p * gy64[:, :n_classes].sum(axis=1, keepdims=True)
                                                    + gy64[:, :n_classes] + d64[:, :n_classes])
    steps = min(chunk, Hs * Ws) + 1
    bx = np.einsum("ck,nchw->nkhw", w64, e_dz) + CH * u * np.einsum("ck,nchw->nkhw", w64, d64)
    bw = np.einsum("nchw,nkhw->ck", e_dz, x64) + steps * u * np.einsum("nchw,nkhw->ck", d64, x64)
    bb = e_dz.sum(axis=(0, 2, 3)) + steps * u * d64.sum(axis=(0, 2, 3))
    return 1.01 * bx, 1.01 * bw, 1.01 * bb


def torch_autograd64(x, w, b, n_classes, target, reg_grad, ignore_index=255):
    """Conv2d 1x1 -> -log_softmax on the classes -> cat, then NLLLoss(mean, ignore_index) on the class planes (as log
    probabilities, i.e. negated back) plus sum(reg_grad * regression planes), all in float64: (loss of the classes,
    dX, dW, db, the logits)."""
    import torch
    C, K = w.shape
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    seg = torch.nn.Conv2d(K, C, kernel_size=1, bias=True).double()
    with torch.no_grad():
        seg.weight.copy_(torch.from_numpy(w.astype(np.float64)).reshape(C, K, 1, 1))
        seg.bias.copy_(torch.from_numpy(b.astype(np.float64)))
    z = seg(xt)
    out = torch.cat((-torch.nn.LogSoftmax(dim=1)(z[:, :n_classes]), z[:, n_classes:]), dim=1)
    closs = torch.nn.NLLLoss(reduction="mean", ignore_index=ignore_index)(-out[:, :n_classes],
                                                                         torch.from_numpy(target.astype(np.int64)))
    total = closs + (out[:, n_classes:] * torch.from_numpy(reg_grad.astype(np.float64))).sum()
    total.backward()
    return (closs.item(), xt.grad.numpy(), seg.weight.grad.numpy().reshape(C, K), seg.bias.grad.numpy(),
            z.detach().numpy())


def zero_class_region(shape):
    """Where random_grad leaves all class planes zero: the last frame of a batch, the first row of a single frame."""
    return (-1,) if shape[0] > 1 else (0, slice(None), 0)


def random_grad(shape, n_classes, seed):
    """A random upstream gradient [n][C][Hs][Ws] fp32 in the normal range: N(0, 1) / 64, a fifth of it exact zeros,
    and the class planes all zero in zero_class_region."""
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal(shape) / 64.0).astype(np.float32)
    g[rng.random(shape) < 0.2] = 0.0
    g[:, :n_classes][zero_class_region(shape)] = 0.0
    return g
