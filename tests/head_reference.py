"""The reference of the segmentation head (is_segmentation_head, instance_stixels_core.h f13), independent of the
kernel: the logits from a C function of a dozen lines, the k-ordered fmaf chain of the contract, compiled with the
host compiler into a temporary directory on first use (-ffp-contract=off; fmaf is the correctly rounded fused
operation of libm or the hardware's); everything behind the logits in numpy float64; the int tensor from
oracle.flip_and_pad."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from oracle import oracle

SOURCE = r"""
#include <math.h>
#include <stddef.h>
/* x [K][P], w [C][K], bias [C] -> z [C][P]: one fp32 chain per (c, p) in increasing k, started from the bias */
void head_logits(const float* x, const float* w, const float* bias, float* z, int C, int K, long P) {
    for (int c = 0; c < C; c++)
        for (long p = 0; p < P; p++) {
            float acc = bias[c];
            for (int k = 0; k < K; k++) acc = fmaf(w[(size_t)c * K + k], x[(size_t)k * P + p], acc);
            z[(size_t)c * P + p] = acc;
        }
}
"""
_LIB = None
_DIR = None


def _lib():
    global _LIB, _DIR
    if _LIB is None:
        _DIR = tempfile.TemporaryDirectory(prefix="head_reference_")
        src, so = os.path.join(_DIR.name, "head_logits.c"), os.path.join(_DIR.name, "libhead_logits.so")
        with open(src, "w") as f:
            f.write(SOURCE)
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", src, "-o", so, "-lm"],
                       check=True)
        _LIB = ctypes.CDLL(so)
        fp = ctypes.POINTER(ctypes.c_float)
        _LIB.head_logits.argtypes = [fp, fp, fp, fp, ctypes.c_int, ctypes.c_int, ctypes.c_long]
        _LIB.head_logits.restype = None
    return _LIB


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def logits(features, weight, bias):
    """features [n][K][Hs][Ws] (any float dtype numpy holds; widened to fp32, exact for halves), weight [C][K],
    bias [C] -> fp32 logits [n][C][Hs][Ws]."""
    x = np.ascontiguousarray(features, np.float32)
    w = np.ascontiguousarray(weight, np.float32)
    b = np.ascontiguousarray(bias, np.float32)
    n, K, Hs, Ws = x.shape
    C = b.size
    assert w.shape == (C, K)
    z = np.empty((n, C, Hs, Ws), np.float32)
    for i in range(n):
        _lib().head_logits(_fp(x[i]), _fp(w), _fp(b), _fp(z[i]), C, K, Hs * Ws)
    return z


def class_values64(z, n_classes):
    """float64 [n][n_classes][Hs][Ws]: (m + log(sum_j exp(z_j - m))) - z_c on the fp32 logits, in binary64."""
    zc = z[:, :n_classes].astype(np.float64)
    m = zc.max(axis=1, keepdims=True)
    lse = m + np.log(np.exp(zc - m).sum(axis=1, keepdims=True))
    return lse - zc


def cnn_out(z, n_classes, clamp=None):
    """The float network output [n][C][Hs][Ws] fp32 of fp32 logits: the class values rounded once, the regression
    channels unchanged but for clamp = (channel, lo, hi)."""
    out = z.copy()
    out[:, :n_classes] = class_values64(z, n_classes).astype(np.float32)
    if clamp is not None:
        c, lo, hi = clamp
        out[:, c] = np.clip(out[:, c], np.float32(lo), np.float32(hi))
    return out


def class_tolerance(z, n_classes):
    """The bound of the class channels, float64 [n][n_classes][Hs][Ws]: ulp_fp32(ref) + 2^-40 (1 + max_c |z_c|)."""
    ref = class_values64(z, n_classes)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    zmax = np.abs(z[:, :n_classes].astype(np.float64)).max(axis=1, keepdims=True)
    return ulp + 2.0 ** -40 * (1.0 + zmax)


def segmentation(cnn, p2s):
    """[n][Ws][C][P2S] int32 of a float output [n][C][Hs][Ws]: oracle.flip_and_pad frame by frame."""
    return np.stack([oracle.flip_and_pad(f, p2s) for f in cnn])


def random_inputs(n, K, Hs, Ws, channels, seed, n_out_init=21):
    """The issue's random inputs: features |N(0, 1)|, weights N(0, sqrt(2 / 21)) (the reference's init of `seg`),
    bias N(0, 0.1); fp32."""
    rng = np.random.default_rng(seed)
    x = np.abs(rng.standard_normal((n, K, Hs, Ws))).astype(np.float32)
    w = (rng.standard_normal((channels, K)) * np.sqrt(2.0 / n_out_init)).astype(np.float32)
    b = (rng.standard_normal(channels) * 0.1).astype(np.float32)
    return x, w, b
