"""is_pack_sections / is_unpack_sections (is_k_pack.hip) at their edges: more than one column per thread of the
scan (n_columns > 1024, ragged), terminators around the 64-lane rounds of the count, the smallest Section
arrays, a partial last workgroup, a batch without any section -- against frontend_reference's restatement,
bytewise, with canaries around every device output and behind what the kernels may write.  Hand-built Sections
with random bytes in every field, so that a half-copied 32-byte record shows."""
import functools

import numpy as np
import pytest

import frontend_reference as fr
from test_render_gpu import Out

N_COLUMNS = (1, 3, 4, 5, 1023, 1024, 1025, 2049, 5003)   # scan: 1, 2, 3 and 5 columns per thread, ragged tails
MAX_SECTIONS = (2, 3, 64, 65, 66, 200)
FILL = 0x5C      # the body of a fresh output (test_render_gpu.Out)
UNPACK_FILL = 0xA5


def _positions(S):
    """Terminator positions of a column: around the 64-lane rounds and both ends; None = no terminator."""
    return sorted({p for p in (0, 1, 62, 63, 64, 65, S - 2, S - 1) if 0 <= p < S}) + [None]


@functools.lru_cache(maxsize=None)
def _sections(n, S, empty=False):
    """[n][S] Sections (read-only) of random bytes with the first terminator of column c at position
    _positions(S)[...] -- every position in turn, then at random -- and, in every second column, a second
    terminator behind the first.  empty: every column starts with its terminator."""
    rng = np.random.default_rng(n * 1009 + S)
    sec = rng.integers(0, 256, (n, S, fr.SECTION_DTYPE.itemsize), dtype=np.uint8).view(fr.SECTION_DTYPE)
    sec = sec.reshape(n, S)
    sec["type"][sec["type"] == -1] = 7
    choices = _positions(S)
    pick = np.concatenate([np.arange(len(choices)), rng.integers(0, len(choices), n)])[:n]
    rng.shuffle(pick)
    for c in range(n):
        p = 0 if empty else choices[pick[c]]
        if p is None:
            continue
        sec["type"][c, p] = -1
        if c % 2 == 0 and p + 1 < S:
            sec["type"][c, rng.integers(p + 1, S)] = -1          # ignored: the first one counts
    sec.setflags(write=False)
    return sec


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


# ---- CPU half ---------------------------------------------------------------------------------------------
def test_section_dtype_is_the_products():
    from instance_stixels_amd.config import SECTION_DTYPE
    assert fr.SECTION_DTYPE == SECTION_DTYPE and fr.SECTION_DTYPE.itemsize == 32


def test_restatement_by_hand():
    sec = np.zeros((4, 3), fr.SECTION_DTYPE)
    sec["vB"] = np.arange(12).reshape(4, 3)
    sec["type"][0, 0] = -1                     # empty
    sec["type"][1, 1] = -1                     # one section
    sec["type"][2, 2] = -1                     # two sections, terminator in the last slot
    counts, offsets, packed = fr.pack_sections(sec)          # column 3: no terminator, capped at S - 1
    assert counts.tolist() == [0, 1, 2, 2] and offsets.tolist() == [0, 0, 1, 3, 5]
    assert packed["vB"].tolist() == [3, 6, 7, 9, 10]
    back = fr.unpack_sections(counts, packed, 3, UNPACK_FILL)
    assert back["type"][[0, 1, 2, 3], counts].tolist() == [-1] * 4
    assert back["vB"][1, 0] == 3 and back["vB"][3, :2].tolist() == [9, 10] and back["vB"][3, 2] == 0
    assert (_bytes(back[0, 1:]) == UNPACK_FILL).all() and (_bytes(back[1, 2:]) == UNPACK_FILL).all()


@pytest.mark.parametrize("n,S", [(5, 2), (1025, 65), (37, 200)])
def test_restatement_equals_the_host_logic(n, S):
    """... of instance_stixels_amd.parallel (torch on CPU tensors), which the gloo tests and
    test_parity_gpu.test_pack_sections_kernels_match_host_logic use."""
    import torch
    from instance_stixels_amd.parallel import pack_sections
    sec = _sections(n, S)
    counts, offsets, packed = fr.pack_sections(sec)
    c_ref, p_ref = pack_sections(torch.from_numpy(np.array(sec).view(np.int32).reshape(n, S, 8)))
    assert np.array_equal(counts, c_ref.numpy()) and offsets[n] == p_ref.shape[0]
    assert np.array_equal(packed.view(np.int32).reshape(-1, 8), p_ref.numpy())
    seen = {int(c) for c in counts}
    assert len(seen) == min(n, len({min(p if p is not None else S, S - 1) for p in _positions(S)}))


# ---- GPU half ---------------------------------------------------------------------------------------------
def _pack(d_sections, n, S, capacity):
    """is_pack_sections into fresh outputs -> (counts, offsets, packed body [capacity])."""
    import torch
    from instance_stixels_amd import core
    counts, offsets = Out((n,), np.int32), Out((n + 1,), np.int32)
    packed = Out((capacity,), fr.SECTION_DTYPE)
    core.pack_sections_ptr(d_sections, n, S, counts.ptr, offsets.ptr, packed.ptr,
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return counts, offsets, packed


def _check(n, S, empty=False):
    import torch
    from instance_stixels_amd import core
    sec = _sections(n, S, empty)
    want_c, want_o, want_p = fr.pack_sections(sec)
    total = int(want_o[n])
    assert total == (0 if empty else int(want_c.sum()))
    capacity = total + 3                       # three records of room: what lies behind `total` stays untouched
    d_sec = torch.from_numpy(np.array(sec).view(np.uint8).reshape(-1)).to(torch.device("cuda", 0))
    assert d_sec.data_ptr() % 16 == 0
    counts, offsets, packed = _pack(d_sec.data_ptr(), n, S, capacity)
    got_c, got_o, got_p = counts.get(), offsets.get(), packed.get()      # (get() checks the canaries around)
    assert np.array_equal(got_c, want_c), np.argwhere(got_c != want_c)[:5].tolist()
    assert np.array_equal(got_o, want_o), np.argwhere(got_o != want_o)[:5].tolist()
    assert np.array_equal(_bytes(got_p[:total]), _bytes(want_p))
    assert (_bytes(got_p[total:]) == FILL).all(), "written behind packed[total]"

    # unpack into 0xA5: slots 0 .. count of every column, and not one byte behind them
    back, offsets2 = Out((n, S), fr.SECTION_DTYPE, fill=UNPACK_FILL), Out((n + 1,), np.int32)
    stream = torch.cuda.current_stream().cuda_stream
    core.unpack_sections_ptr(counts.ptr, offsets2.ptr, packed.ptr, n, S, back.ptr, stream)
    torch.cuda.synchronize()
    assert np.array_equal(offsets2.get(), want_o)
    assert np.array_equal(counts.get(), want_c) and np.array_equal(_bytes(packed.get()), _bytes(got_p))
    got_b, want_b = back.get(), fr.unpack_sections(want_c, want_p, S, UNPACK_FILL)
    diff = (got_b.view(np.uint8).reshape(n, S, -1) != want_b.view(np.uint8).reshape(n, S, -1)).any(axis=2)
    assert not diff.any(), [(c, s, int(want_c[c])) for c, s in np.argwhere(diff)[:5].tolist()]

    # pack(unpack(pack(x))) = pack(x)
    counts3, offsets3, packed3 = _pack(back.ptr, n, S, capacity)
    assert np.array_equal(counts3.get(), want_c) and np.array_equal(offsets3.get(), want_o)
    got_p3 = packed3.get()
    assert np.array_equal(_bytes(got_p3[:total]), _bytes(want_p)) and (_bytes(got_p3[total:]) == FILL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("S", MAX_SECTIONS)
@pytest.mark.parametrize("n", N_COLUMNS)
def test_pack_and_unpack_equal_the_restatement(n, S):
    _check(n, S)


@pytest.mark.gpu
def test_a_batch_without_sections_writes_nothing():
    _check(1025, 65, empty=True)
