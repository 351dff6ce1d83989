"""The reference of the CNN label maps (is_cnn_label_maps, instance_stixels_core.h f15), independent of the kernel:
the contract as a C loop, compiled with the host compiler into a temporary directory on first use
(-ffp-contract=off; fmaf is the correctly rounded fused operation of libm or the hardware's), and numpy for the
class -> label table and the confusion table.  The weights are the contract's one-line formula."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

SOURCE = r"""
#include <math.h>
#include <stddef.h>
#include <stdint.h>
static int first_min(const float* v, int n) {
    int best = 0;
    for (int c = 1; c < n; c++)
        if (v[c] < v[best]) best = c;
    return best;
}
static float W(int k) { return (float)(2 * (k < 15 - k ? k : 15 - k) + 1) / 16.0f; }
/* planes [C][Hs][Ws] of one frame -> class8 [Hs][Ws], cls [8 Hs][8 Ws] (the class of every pixel) and, when up is
 * given, up [C][8 Hs][8 Ws]: the upsampled values of mode 1 (the planes' own values repeated in mode 0) */
void cnn_classes(const float* planes, int C, int Hs, int Ws, int mode, uint8_t* class8, uint8_t* cls, float* up) {
    float v[64];
    const int H = 8 * Hs, Wd = 8 * Ws;
    for (int y = 0; y < Hs; y++)
        for (int x = 0; x < Ws; x++) {
            for (int c = 0; c < C; c++) v[c] = planes[((size_t)c * Hs + y) * Ws + x];
            class8[y * Ws + x] = (uint8_t)first_min(v, C);
        }
    for (int Y = 0; Y < H; Y++)
        for (int X = 0; X < Wd; X++) {
            for (int c = 0; c < C; c++) {
                const float* p = planes + (size_t)c * Hs * Ws;
                if (mode == 0) {
                    v[c] = p[(Y / 8) * Ws + X / 8];
                } else {
                    float acc = 0.0f;
                    for (int iy = (Y + 4) / 8 - 1; iy <= (Y + 4) / 8; iy++)
                        for (int ix = (X + 4) / 8 - 1; ix <= (X + 4) / 8; ix++) {
                            if (iy < 0 || iy >= Hs || ix < 0 || ix >= Ws) continue; /* skipped, not times zero */
                            acc = fmaf(W(Y + 4 - 8 * iy) * W(X + 4 - 8 * ix), p[iy * Ws + ix], acc);
                        }
                    v[c] = acc;
                }
                if (up) up[((size_t)c * H + Y) * Wd + X] = v[c];
            }
            cls[(size_t)Y * Wd + X] = (uint8_t)first_min(v, C);
        }
}
"""
_LIB = None
_DIR = None
NEAREST, DECONV = 0, 1
MODES = {"nearest": NEAREST, "deconv": DECONV}
CITYSCAPES = np.array([7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33], np.uint8)


def _lib():
    global _LIB, _DIR
    if _LIB is None:
        _DIR = tempfile.TemporaryDirectory(prefix="cnn_labels_reference_")
        src, so = os.path.join(_DIR.name, "cnn_classes.c"), os.path.join(_DIR.name, "libcnn_classes.so")
        with open(src, "w") as f:
            f.write(SOURCE)
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", src, "-o", so, "-lm"],
                       check=True)
        _LIB = ctypes.CDLL(so)
        fp, bp, ci = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint8), ctypes.c_int
        _LIB.cnn_classes.argtypes = [fp, ci, ci, ci, ci, bp, bp, fp]
        _LIB.cnn_classes.restype = None
    return _LIB


def weights():
    """The 16 one-dimensional tap weights W[k] = (2 min(k, 15 - k) + 1) / 16, fp32."""
    k = np.arange(16)
    return ((2 * np.minimum(k, 15 - k) + 1) / 16.0).astype(np.float32)


def classes(cnn_out, n_classes, mode, want_values=False):
    """cnn_out [n][channels >= n_classes][Hs][Ws] fp32 -> (class8 [n][Hs][Ws], pixel classes [n][8 Hs][8 Ws]) uint8,
    and with want_values the upsampled fp32 values [n][n_classes][8 Hs][8 Ws] in third place."""
    x = np.ascontiguousarray(np.asarray(cnn_out, np.float32)[:, :n_classes])
    n, C, Hs, Ws = x.shape
    c8 = np.empty((n, Hs, Ws), np.uint8)
    cls = np.empty((n, 8 * Hs, 8 * Ws), np.uint8)
    up = np.empty((n, C, 8 * Hs, 8 * Ws), np.float32) if want_values else None
    fp, bp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint8)
    for i in range(n):
        _lib().cnn_classes(x[i].ctypes.data_as(fp), C, Hs, Ws, MODES.get(mode, mode), c8[i].ctypes.data_as(bp),
                           cls[i].ctypes.data_as(bp), up[i].ctypes.data_as(fp) if want_values else None)
    return (c8, cls, up) if want_values else (c8, cls)


def table(n_classes, class_to_label=None):
    """The class -> label table of a call, uint8 [n_classes]: the caller's, or Cityscapes trainId -> labelId (19
    entries); a class outside the table gives 0."""
    t = np.zeros(n_classes, np.uint8)
    src = CITYSCAPES if class_to_label is None else np.asarray(class_to_label, np.uint8)
    k = min(n_classes, src.size)
    t[:k] = src[:k]
    return t


def label_maps(cnn_out, n_classes, mode, cols=None, class_to_label=None):
    """(class8, label [n][8 Hs][cols]): the label image of the contract, 0 in the margin X >= 8 Ws."""
    c8, cls = classes(cnn_out, n_classes, mode)
    n, H, Wd = cls.shape
    cols = Wd if cols is None else cols
    label = np.zeros((n, H, cols), np.uint8)
    label[:, :, :Wd] = table(n_classes, class_to_label)[cls]
    return c8, label


def confusion(label, gt, n_labels, width, start=None):
    """conf[gt][pred] += 1 over the pixels with X < width, gt < n_labels and pred < n_labels; uint64
    [n_labels][n_labels], added to `start`."""
    p = label[:, :, :width].astype(np.int64).ravel()
    g = gt[:, :, :width].astype(np.int64).ravel()
    ok = (p < n_labels) & (g < n_labels)
    conf = np.bincount(g[ok] * n_labels + p[ok], minlength=n_labels * n_labels).reshape(n_labels, n_labels)
    conf = conf.astype(np.uint64)
    return conf if start is None else conf + np.asarray(start, np.uint64)


def random_costs(n, channels, Hs, Ws, seed, n_classes=19, sigma=3.0):
    """-log_softmax of N(0, sigma) logits in the class planes (float64, rounded once), N(0, 1) in the others."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, channels, Hs, Ws))
    zc = z[:, :n_classes] * sigma
    m = zc.max(axis=1, keepdims=True)
    z[:, :n_classes] = (m + np.log(np.exp(zc - m).sum(axis=1, keepdims=True))) - zc
    return z.astype(np.float32)
