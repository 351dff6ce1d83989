"""The reference of the full-resolution semantic NLL through the `up` layer (is_semantic_nll_up,
instance_stixels_core.h f16), independent of the kernel: numpy float64, evaluated on the fp32 chain values u that
cnn_labels_reference.classes(..., want_values=True) returns, so that the upsampling's rounding is in no tolerance.
The gradient is the explicit transposed operator with the contract's skipped taps.

The bounds of the device's fp32 operation sequence (header f16, eps = 2^-24, an error of k ulp <= 2 k eps relative):
  S      the sum of C terms expf(m - u_c) in (0, 1], the largest 1: C - 1 additions, each term off by 2 K_EXP eps and
         by the rounding of its argument, |d| e^d eps <= eps / e.  rel(S) <= (C - 1 + 2 K_EXP + C / e) eps =: RS eps
  K      m - logf(S): |dK| <= (|K| + 2 K_LOG |log S| + RS) eps
  L_pix  u_t - K: |dL| <= |dK| + |L| eps
  p_c    expf(K - u_c): |dp| <= p (2 K_EXP + |K - u_c|) eps + p |dK|
  r_c    [c == t] - p_c: |dr| <= |dp| + [c == t] |r| eps
  cell   8 fmaf of the row sum, 8 of the column sum, 3 additions, the product with inv_V and inv_V's own rounding: 21
         roundings of partial sums that sum W W |r| bounds, plus the operator on |dr|; all times inv_V
  loss   the per-pixel |dL| averaged, the binary64 sum's floor 2^-40 mean |L|, one fp32 ulp of the result
Every bound is multiplied by 1.01 for the second-order terms; the gradient's has a floor of 1024 * 2^-149 for results
in the subnormal range.  K_EXP = K_LOG = 3: the OpenCL C specification's bounds for exp and log (<= 3 ulp), which the
ROCm device library's expf and logf are built to."""
import numpy as np

import cnn_labels_reference as cr

K_EXP = 3
K_LOG = 3
EPS = 2.0 ** -24


def operator(n_cells):
    """A [n_cells][8 n_cells]: A[i, o] = W[o + 4 - 8 i] where that tap exists.  up(v) = A_y^T v A_x, with taps outside
    the plane skipped; the gradient's operator is A_y r A_x^T."""
    W = cr.weights().astype(np.float64)
    A = np.zeros((n_cells, 8 * n_cells))
    for i in range(n_cells):
        for k in range(16):
            o = 8 * i + k - 4
            if 0 <= o < 8 * n_cells:
                A[i, o] = W[k]
    return A


def transposed(r):
    """[..][8 Hs][8 Ws] -> [..][Hs][Ws]: sum W[ky] W[kx] r over each cell's footprint inside the image."""
    H, Wd = r.shape[-2:]
    return operator(H // 8) @ r @ operator(Wd // 8).T


def from_values(u, target, ignore_index=255):
    """u [n][C][H][Wd] float64, the upsampled values; target [n][H][cols >= Wd] of integers.  A dict: per-pixel loss
    (0 where the pixel does not count), loss (float64; NaN without a valid pixel), valid, bad, grad [n][C][H/8][Wd/8]
    float64, and the quantities the bounds are made of."""
    u = np.asarray(u, np.float64)
    n, C, H, Wd = u.shape
    t = np.asarray(target)[:, :, :Wd].astype(np.int64)
    cls = (t >= 0) & (t < C) & (t != ignore_index)
    bad = ~cls & (t != ignore_index)
    m = u.min(axis=1)
    S = np.exp(m[:, None] - u).sum(axis=1)
    logS = np.log(S)
    K = m - logS
    ut = np.take_along_axis(u, np.where(cls, t, 0)[:, None], axis=1)[:, 0]
    L = np.where(cls, ut - K, 0.0)
    V = int(cls.sum())
    p = np.exp(K[:, None] - u)
    onehot = (np.arange(C)[None, :, None, None] == t[:, None]) & cls[:, None]
    r = (onehot - p) * cls[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = L.sum() / V if V else np.nan
    grad = transposed(r) / V if V else np.zeros((n, C, H // 8, Wd // 8))
    return dict(u=u, pixel_loss=L, loss=loss, valid=V, bad=int(bad.sum()), grad=grad, K=K, logS=logS, p=p, r=r,
                onehot=onehot, counts=cls)


def evaluate(cnn_out, target, n_classes, ignore_index=255):
    """cnn_out [n][channels >= n_classes][Hs][Ws] fp32: from_values on f15's fp32 chain values."""
    up = cr.classes(cnn_out, n_classes, "deconv", want_values=True)[2]
    return from_values(up, target, ignore_index)


def _rs(C):
    return C - 1 + 2 * K_EXP + C / np.e


def loss_bound(ref):
    """|device loss - ref['loss']| of the fp32 sequence (see the module's docstring)."""
    C, V = ref["u"].shape[1], ref["valid"]
    dK = (np.abs(ref["K"]) + 2 * K_LOG * np.abs(ref["logS"]) + _rs(C)) * EPS
    dL = np.where(ref["counts"], dK + np.abs(ref["pixel_loss"]) * EPS, 0.0)
    mean_abs = np.abs(ref["pixel_loss"]).sum() / V
    return 1.01 * (dL.sum() / V + 2.0 ** -40 * mean_abs) + float(np.spacing(np.float32(abs(ref["loss"]))))


def grad_bound(ref):
    """|device grad - ref['grad']| per element of the fp32 sequence (see the module's docstring)."""
    C, V = ref["u"].shape[1], ref["valid"]
    K, u, p, r = ref["K"][:, None], ref["u"], ref["p"], ref["r"]
    counts = ref["counts"][:, None]
    dK = (np.abs(K) + 2 * K_LOG * np.abs(ref["logS"][:, None]) + _rs(C)) * EPS
    dp = p * ((2 * K_EXP + np.abs(K - u)) * EPS + dK)
    dr = np.where(counts, dp + ref["onehot"] * np.abs(r) * EPS, 0.0)
    return 1.01 * transposed(21 * EPS * np.abs(r) + dr) / V + 1024 * 2.0 ** -149


def random_targets(n, rows, cols, n_classes, seed, ignore_index=255, ignored=0.1, block=16):
    """Class ids constant in block x block squares with a share of ignore_index, as label images are."""
    rng = np.random.default_rng(seed)
    hb, wb = (rows + block - 1) // block, (cols + block - 1) // block
    t = rng.integers(0, n_classes, (n, hb, wb))
    t[rng.random((n, hb, wb)) < ignored] = ignore_index
    t = np.repeat(np.repeat(t, block, axis=1), block, axis=2)[:, :rows, :cols]
    return np.ascontiguousarray(t.astype(np.uint8))
