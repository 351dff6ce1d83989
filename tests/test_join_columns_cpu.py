"""JoinColumns at its edges, CPU half: the inputs of tests/test_join_columns_gpu.py, the conditions they must
meet, and the restatement (frontend_reference.join_columns) against oracle.join_columns on every one of them.

The inputs: unaligned image widths and margins, every valid count 0..8 of a group, median ties, -0.0 next to
an invalid value of 0.0, and a sprinkling of NaN, +-inf and negative values."""
import functools

import numpy as np
import pytest

import frontend_reference as fr
from instance_stixels_amd import make_config
from oracle import oracle

D = 32
N_IMAGES = 3
STEP = 8
PRESET = "drn_d_22_unary"
# name: (rows, full_cols, width_margin, realcols)
CASES = {
    "width67": (72, 67, 0, 8),        # width % 4 = 3: the row starts cycle through all four alignments
    "margin3": (64, 131, 3, 16),      # odd margin
    "tiles": (136, 270, 6, 33),       # 33 columns cross the 32-column tile, 136 rows two 64-row tiles
    "one": (8, 9, 1, 1),              # one column, the smallest legal row count
    "aligned": (64, 256, 0, 32),      # every group 16-byte aligned (control)
}
INVALIDS = (-1.0, 0.0, 5.0)
# Groups per valid count 0..8 that an input with invalid >= 0 must hold.  "one" has 3 * 8 * 1 = 24 groups in
# all, fewer than 9 * 20: there every count occurs once and the other cases carry the numbers.
MIN_PER_COUNT = {"width67": 20, "margin3": 20, "tiles": 20, "one": 1, "aligned": 20}


def config(name, invalid, median):
    rows, full_cols, margin, realcols = CASES[name]
    cfg = make_config(PRESET, rows, full_cols, D, width_margin=margin, invalid_disparity=invalid,
                      median_join=median)
    assert cfg.realcols == realcols
    return cfg


@functools.lru_cache(maxsize=None)
def make_input(name, invalid, sprinkle=True):
    """[N_IMAGES][rows][full_cols] fp32 (read-only): a random field in [0, D) with hand-made groups in it, every
    kind in groups of its own.  sprinkle=False leaves out NaN, +-inf and the negative values."""
    rows, full_cols, margin, realcols = CASES[name]
    rng = np.random.default_rng(1000 + 7 * list(CASES).index(name))
    big = rng.random((N_IMAGES, rows, full_cols), dtype=np.float32) * np.float32(D)
    n_groups = N_IMAGES * rows * realcols
    order = iter(rng.permutation(n_groups))
    small = n_groups < 1000

    def take(k):
        for _ in range(k):
            img, rem = divmod(int(next(order)), rows * realcols)
            row, c = divmod(rem, realcols)
            yield big[img, row, margin + c * STEP: margin + (c + 1) * STEP]       # a view of the group

    if invalid >= 0:
        for count in range(STEP + 1):                          # groups with exactly `count` valid values
            for g in take(1 if small else 24):
                g[rng.permutation(STEP)[:STEP - count]] = invalid
    for g in take(1 if small else 4):                          # median ties: all equal
        g[:] = g[0]
    for g in take(1 if small else 4):                          # ... and two distinct values four times each
        g[:] = rng.permutation(np.repeat(g[:2], 4))
    patterns = ([-0.0, 0.0, -0.0, 7.5, 0.25, 0.0, -0.0, 3.0], [-0.0] * 8, [-0.0, 0.0] * 4,
                [0.0, -0.0, -0.0, 0.0, -0.0, 0.0, 0.0, -0.0], [-0.0, 1.0, -0.0, 2.0, -0.0, 3.0, -0.0, 4.0],
                [0.0] * 7 + [-0.0])
    for k, g in enumerate(take(1 if small else 6)):            # -0.0: invalid when invalid == 0.0
        g[:] = patterns[k]
    if sprinkle:
        specials = (np.nan, np.inf, -np.inf)
        for k, g in enumerate(take(max(1, n_groups // 100))):  # about 1 % of the groups hold non-finite values
            g[rng.integers(0, STEP)] = specials[k % 3]
            if k % 4 == 3:
                g[rng.integers(0, STEP)] = specials[(k // 4) % 3]
        for k, g in enumerate(take(max(1, n_groups // 100))):  # negative values, -1.0 among them
            pos = rng.permutation(STEP)[:1 + k % 3]
            g[pos] = -rng.random(pos.size, dtype=np.float32) * np.float32(D)
            if k % 2 == 0:
                g[pos[0]] = -1.0
    big.setflags(write=False)
    return big


def groups(name, big):
    """[N_IMAGES][rows][realcols][STEP] view of the groups of an input."""
    rows, full_cols, margin, realcols = CASES[name]
    return big[:, :, margin: margin + realcols * STEP].reshape(N_IMAGES, rows, realcols, STEP)


@functools.lru_cache(maxsize=None)
def restatement(name, invalid, median, sprinkle=True):
    """[N_IMAGES][realcols][rows] of frontend_reference.join_columns on make_input (computed once, read-only)."""
    rows, full_cols, margin, realcols = CASES[name]
    big = make_input(name, invalid, sprinkle)
    out = np.stack([fr.join_columns(big[i], rows, full_cols, realcols, margin, median, invalid)
                    for i in range(N_IMAGES)])
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("invalid", INVALIDS)
@pytest.mark.parametrize("name", list(CASES))
def test_inputs_hold_what_they_are_for(name, invalid):
    big = make_input(name, invalid)
    g = groups(name, big)
    assert (big[np.isfinite(big)] < D).all()
    if invalid >= 0:
        valid = (g != np.float32(invalid)).sum(axis=3)
        hist = np.bincount(valid.ravel(), minlength=STEP + 1)
        print(f"{name} invalid {invalid}: groups per valid count 0..8 {hist.tolist()}")
        assert (hist >= MIN_PER_COUNT[name]).all(), hist
    flat = g.reshape(-1, STEP)
    assert (flat == flat[:, :1]).all(axis=1).any()                                   # all equal
    srt = np.sort(flat, axis=1)
    assert ((srt[:, 0] == srt[:, 3]) & (srt[:, 4] == srt[:, 7]) & (srt[:, 3] != srt[:, 4])).any()   # 4 + 4
    assert ((flat == 0) & np.signbit(flat)).any()                                    # -0.0
    assert np.isnan(big).any() and (big < 0).any() and (big == -1.0).any()
    if name != "one":                                # (its 24 groups leave room for one non-finite group)
        assert (big == np.inf).any() and (big == -np.inf).any()
    clean = make_input(name, invalid, sprinkle=False)
    assert np.isfinite(clean).all() and not (clean < 0).any()
    for median in (False, True):
        out = restatement(name, invalid, median)
        finite = float(np.isfinite(out).mean())
        print(f"{name} invalid {invalid} median {median}: finite outputs {finite:.4f}")
        assert finite >= 0.95
        assert median or not np.isfinite(out).all()  # (a median may step over a NaN; a mean cannot)


@pytest.mark.parametrize("sprinkle", [True, False])
@pytest.mark.parametrize("median", [False, True])
@pytest.mark.parametrize("invalid", INVALIDS)
@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_the_oracle(name, invalid, median, sprinkle):
    big = make_input(name, invalid, sprinkle)
    cfg = config(name, invalid, median)
    want = restatement(name, invalid, median, sprinkle)
    assert want.shape == (N_IMAGES, cfg.realcols, cfg.rows) and want.dtype == np.float32
    for i in range(N_IMAGES):
        assert fr.same_floats(want[i], oracle.join_columns(cfg, big[i])), i


def test_same_floats_is_bitwise_apart_from_nan():
    a = np.array([0.0, 1.0, np.nan, np.inf], np.float32)
    assert fr.same_floats(a, a.copy())
    assert not fr.same_floats(a, np.array([-0.0, 1.0, np.nan, np.inf], np.float32))
    assert not fr.same_floats(a, np.array([0.0, 1.0, 2.0, np.inf], np.float32))
    b = a.copy()
    b.view(np.uint32)[2] ^= 1                       # another NaN payload
    assert np.isnan(b[2]) and fr.same_floats(a, b)
    assert not fr.same_floats(a, np.nextafter(a, np.float32(2)))
