"""A numpy restatement of f11 (is_mode_downsample, is_gt_instance_targets of include/instance_stixels_core.h): the
reference's ModeDownsample(8) (tools/CNN_training/datasets/transforms.py:59-70), the regression targets of its
training (datasets/cityscapes.py _instance_offsets :146-167, _instance_offsets_disparity :114-144) and the same values
as channels 19 and 20 of a DP input (inference.py:393-396 followed by FlipAndPad, models/wrappers.py:35-61).
Vectorised; tests/golden/reference_python_targets pins it on the reference's own Python."""
import numpy as np

CHANNELS = 21


def mode_downsample(img):
    """[..., rows, cols] -> [..., rows / 8, cols / 8] of the same dtype: the most frequent value of every 8x8 block,
    the smallest among equals (np.bincount(..).argmax()); values compared as the signed / unsigned integers they
    are."""
    img = np.asarray(img)
    rows, cols = img.shape[-2:]
    if rows % 8 or cols % 8 or rows < 8 or cols < 8:
        raise ValueError("rows and cols must be multiples of 8")
    lead = img.shape[:-2]
    Hs, Ws = rows // 8, cols // 8
    b = img.reshape(lead + (Hs, 8, Ws, 8))
    b = np.moveaxis(b, -3, -2).reshape(lead + (Hs, Ws, 64))
    s = np.sort(b, axis=-1)
    at = np.arange(64)
    new = np.ones(s.shape, bool)
    new[..., 1:] = s[..., 1:] != s[..., :-1]
    last = np.ones(s.shape, bool)
    last[..., :-1] = new[..., 1:]
    start = np.maximum.accumulate(np.where(new, at, 0), axis=-1)
    end = np.minimum.accumulate(np.where(last, at, 63)[..., ::-1], axis=-1)[..., ::-1]
    count = end - start + 1
    best = np.argmax(count, axis=-1)   # the first of the longest runs: the smallest value
    return np.take_along_axis(s, best[..., None], axis=-1)[..., 0]


def _keys(ids8):
    """The keyed cells of one frame: (rows, columns, index of each cell's key, the keys in ascending order)."""
    y, x = np.nonzero(ids8 > 1000)
    keys, inv = np.unique(ids8[y, x], return_inverse=True)
    return y, x, inv.reshape(-1), keys


def offsets(ids8):
    """[Hs][Ws] downsampled ids -> float32 [2][Hs][Ws]: (off_y, off_x) of every cell with a key, 0 elsewhere.  The
    sums are integers; one division and one subtraction in float32."""
    ids8 = np.asarray(ids8)
    out = np.zeros((2,) + ids8.shape, np.float32)
    y, x, inv, keys = _keys(ids8)
    if keys.size == 0:
        return out
    n = np.bincount(inv, minlength=keys.size).astype(np.int64)
    sy = np.bincount(inv, weights=y, minlength=keys.size).astype(np.int64)   # (exact: far below 2^53)
    sx = np.bincount(inv, weights=x, minlength=keys.size).astype(np.int64)
    nf = n.astype(np.float32)
    out[0, y, x] = (sy.astype(np.float32) / nf)[inv] - y.astype(np.float32)
    out[1, y, x] = (sx.astype(np.float32) / nf)[inv] - x.astype(np.float32)
    return out


def disparity_plane(ids8, disp8):
    """[Hs][Ws] downsampled ids and downsampled raw uint16 disparity -> float32 [Hs][Ws]: per key the LOWER median
    (torch.median) of its non-zero q = v // 256, 0 where it has none, in every cell of the key."""
    ids8 = np.asarray(ids8)
    q = np.asarray(disp8).astype(np.int64) // 256
    out = np.zeros(ids8.shape, np.float32)
    y, x, inv, keys = _keys(ids8)
    if keys.size == 0:
        return out
    qq = q[y, x]
    live = qq != 0
    order = np.lexsort((qq[live], inv[live]))
    sk, sq = inv[live][order], qq[live][order]
    c = np.bincount(sk, minlength=keys.size)
    first = np.concatenate(([0], np.cumsum(c)[:-1]))
    median = np.zeros(keys.size, np.int64)
    has = c > 0
    median[has] = sq[(first + (c - 1) // 2)[has]]
    out[y, x] = median[inv].astype(np.float32)
    return out


def key_counts(ids8):
    """[n][Hs][Ws] -> the distinct keys of every frame."""
    return np.array([np.unique(f[f > 1000]).size for f in np.asarray(ids8)], np.int32)


def targets(gt, disparity_u16=None):
    """[n][rows][cols] int32 (and uint16) -> (float32 [n][2 or 3][Hs][Ws], int32 [n][Hs][Ws] downsampled ids)."""
    ids8 = mode_downsample(np.asarray(gt, np.int32))
    planes = []
    d8 = mode_downsample(np.asarray(disparity_u16, np.uint16)) if disparity_u16 is not None else None
    for f in range(ids8.shape[0]):
        off = offsets(ids8[f])
        if d8 is not None:
            off = np.concatenate([disparity_plane(ids8[f], d8[f])[None], off])
        planes.append(off)
    return np.stack(planes), ids8


def as_prediction(segmentation, off):
    """A copy of segmentation [n][Ws][21][P2S] int32 with channels 19 and 20 rewritten from off [n][2][Hs][Ws]
    (off_y, off_x): seg[f][x][19 + k][Hs-1-y] = (int32)(8.0f * off[f][k][y][x]), truncated toward zero; rows Hs .. P2S-1
    of both channels 0; the class channels untouched."""
    seg = np.array(segmentation, np.int32, copy=True)
    n, two, Hs, Ws = off.shape
    assert two == 2 and seg.shape[:3] == (n, Ws, CHANNELS) and seg.shape[3] > Hs
    v = (np.float32(8.0) * off.astype(np.float32)).astype(np.int32)      # [n][2][Hs][Ws]
    seg[:, :, CHANNELS - 2:, :] = 0
    seg[:, :, CHANNELS - 2:, :Hs] = v[:, :, ::-1, :].transpose(0, 3, 1, 2)
    return seg
