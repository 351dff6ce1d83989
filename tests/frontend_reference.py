"""Plain restatements of the small kernels in front of and behind the DP: JoinColumns (k_join_columns), the
v-disparity histogram of the road estimation (k_road_histogram / k_road_binarize) and the
compaction of the Section arrays (is_k_pack.hip).  numpy and Python only, fp32 in the kernels' operation
order, no import from the product: the tests compare the device with these, bit for bit."""
import numpy as np

F32 = np.float32

# Section, include/InstanceStixels/types.h:186-194 of the reference: eight 4-byte fields
SECTION_DTYPE = np.dtype([
    ("type", np.int32), ("vB", np.int32), ("vT", np.int32), ("disparity", np.float32),
    ("semantic_class", np.int32), ("cost", np.float32), ("instance_meanx", np.float32),
    ("instance_meany", np.float32),
])


# ---- JoinColumns (reference StixelsKernels.cu:980-1095) ---------------------------------------------------
def _median(values):
    """The partial selection sort of the reference (:1007-1022): `<` on IEEE values (false for NaN, and for
    -0.0 against 0.0), the middle element, or the fp32 mean of the two middle ones.  Python floats hold every
    fp32 value exactly, so the comparisons are the fp32 ones."""
    t = [float(v) for v in values]
    n = len(t)
    for i in range(n // 2 + 1):
        m = i
        for j in range(i + 1, n):
            if t[j] < t[m]:
                m = j
        t[i], t[m] = t[m], t[i]
    if n % 2 == 0:
        with np.errstate(all="ignore"):
            return (F32(t[n // 2]) + F32(t[n // 2 - 1])) / F32(2.0)
    return F32(t[n // 2])


def join_columns(big, rows, full_cols, realcols, margin, median, invalid, step=8):
    """big [rows][full_cols] fp32 -> [realcols][rows], rows flipped.  Group (row, c) is
    big[row, margin + c*step : margin + (c+1)*step].  Mean: sequential fp32 sum in index order, one fp32
    divide.  invalid >= 0: values == invalid (IEEE compare) are skipped, the divisor is the valid count, a
    group without valid values gives `invalid`.  Median: over the valid values only."""
    big = np.ascontiguousarray(big, F32)
    assert big.shape == (rows, full_cols) and margin + realcols * step <= full_cols
    invalid = F32(invalid)
    g = np.stack([big[:, margin + c * step: margin + (c + 1) * step] for c in range(realcols)], axis=1)
    valid = (g != invalid) if invalid >= 0 else np.ones(g.shape, bool)        # [rows][realcols][step]
    out = np.empty((rows, realcols), F32)
    if median:
        for r in range(rows):
            for c in range(realcols):
                v = g[r, c][valid[r, c]]
                out[r, c] = _median(v) if v.size else invalid
    else:
        with np.errstate(all="ignore"):
            acc = np.zeros((rows, realcols), F32)
            for i in range(step):
                acc = np.where(valid[..., i], acc + g[..., i], acc)            # fp32 + fp32, in index order
            count = valid.sum(axis=2)
            out = np.where(count > 0, acc / np.maximum(count, 1).astype(F32), invalid).astype(F32)
    return np.ascontiguousarray(out[::-1].T)


def same_floats(a, b):
    """Bitwise equality of two fp32 arrays, except that NaN equals NaN whatever its payload."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    if a.shape != b.shape:
        return False
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


# ---- v-disparity (reference RoadEstimationKernels.cu:25-60) -----------------------------------------------
def vdisparity_bins(d, max_dis):
    """Bin of every pixel, -1 where it counts nowhere.  A pixel counts iff d != 0 and its bin is in
    [0, max_dis).  The bin is the truncation toward zero for finite |d| < 2^31; +-inf and |d| >= 2^31 have no
    bin; NaN goes to bin 0 (the reference's float -> int conversion of NaN gives 0 on its GPU).  So values in
    (-1, 0) land in bin 0 and values <= -1 nowhere."""
    d = np.ascontiguousarray(d, F32)
    nan = np.isnan(d)
    convertible = np.isfinite(d) & (np.abs(d.astype(np.float64)) < 2.0 ** 31)
    b = np.full(d.shape, -1, np.int64)
    b[convertible] = np.trunc(d[convertible].astype(np.float64)).astype(np.int64)
    b[nan] = 0
    counts = (d != 0) & (nan | convertible) & (b >= 0) & (b < max_dis)         # NaN != 0 holds
    return np.where(counts, b, -1)


def vdisparity(d, max_dis, threshold):
    """-> (histogram [rows][max_dis] int32, binary [rows][max_dis] uint8, maximum).  Binarisation:
    float32(count) > float32(maximum) * float32(threshold) gives 255."""
    d = np.ascontiguousarray(d, F32)
    rows = d.shape[0]
    b = vdisparity_bins(d, max_dis)
    r = np.nonzero(b >= 0)[0]
    v = np.bincount(r * max_dis + b[b >= 0], minlength=rows * max_dis).astype(np.int32).reshape(rows, max_dis)
    m = int(v.max())
    binary = np.where(v.astype(F32) > F32(m) * F32(threshold), 255, 0).astype(np.uint8)
    return v, binary, m


# ---- compaction of the Section arrays (is_pack_sections / is_unpack_sections) ------------------------------
def pack_sections(sections):
    """sections [n][S] SECTION_DTYPE -> (counts [n] int32, offsets [n + 1] int32, packed [total]).
    count = index of the first type == -1, capped at S - 1 (also without any terminator); offsets = exclusive
    prefix of the counts with the total in entry n; packed = the used sections in column order."""
    n, S = sections.shape
    counts = np.empty(n, np.int32)
    for c in range(n):
        term = np.nonzero(sections["type"][c] == -1)[0]
        counts[c] = min(int(term[0]) if term.size else S, S - 1)
    offsets = np.zeros(n + 1, np.int32)
    offsets[1:] = np.cumsum(counts, dtype=np.int64)
    packed = np.concatenate([sections[c, :counts[c]] for c in range(n)]) if n else sections[:0, 0]
    return counts, offsets, np.ascontiguousarray(packed)


def unpack_sections(counts, packed, S, fill):
    """-> [n][S] SECTION_DTYPE: every byte `fill`, then the `count` sections of each column and the
    terminator (-1, 0, ..., 0) at slot `count`; nothing behind it is touched."""
    n = counts.size
    out = np.full((n, S, SECTION_DTYPE.itemsize), fill, np.uint8).view(SECTION_DTYPE).reshape(n, S)
    term = np.zeros((), SECTION_DTYPE)
    term["type"] = -1
    o = 0
    for c in range(n):
        k = int(counts[c])
        out[c, :k] = packed[o:o + k]
        out[c, k] = term
        o += k
    return out
