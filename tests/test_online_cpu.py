"""No-GPU checks of the online rings (coupe.dvsg_amd.online): the slot rule of `stream_window_row` restates
eval.py:93-124 exactly as `window_index_table` does for a whole clip, and the three entry points behind it reject bad
arguments with a status code before any device work."""
import numpy as np
import pytest

from coupe.dvsg_amd.clip import SKIP_LENGTH, window_index_table
from coupe.dvsg_amd.online import stream_window_row


def _simulate(n, skip_length, base):
    """Run the rings with symbolic frames: each step writes "unstable k" into its input slot, reads the row, then writes
    "stab k" into its out slot.  Returns the frame identities every row named, as the pool indices of
    window_index_table's 2N-frame pool (unstable k -> k, stab j -> N + j)."""
    span = skip_length[-1]
    pool = {}
    named = np.empty((n, len(skip_length)), dtype=np.int64)
    for k in range(n):
        row, out = stream_window_row(k, base, skip_length)
        assert row.dtype == np.int32 and row.shape == (len(skip_length),)
        assert all(base <= r < base + span + 2 for r in row) and base <= out <= base + span
        assert row[-1] == base + span + 1
        pool[base + span + 1] = ("unstable", k)
        for s, r in enumerate(row):
            kind, j = pool[int(r)]
            named[k, s] = j if kind == "unstable" else n + j
        assert out not in row, "step %d reads the history slot it writes" % k
        pool[out] = ("stab", k)
    return named


@pytest.mark.parametrize("skip_length", [SKIP_LENGTH, (0, 2, 3)])
@pytest.mark.parametrize("n", [1, 2, 33, 34, 35, 100])
def test_ring_rows_name_the_frames_of_the_clip_table(n, skip_length):
    for base in (0, 34, 7):
        assert np.array_equal(_simulate(n, skip_length, base), window_index_table(n, skip_length))


def test_ring_rule_first_steps():
    row, out = stream_window_row(0, 0)
    assert list(row) == [33] * 7 and out == 0
    row, out = stream_window_row(1, 0)
    assert list(row) == [0, 0, 0, 0, 0, 0, 33] and out == 1
    row, out = stream_window_row(33, 68)
    assert list(row) == [68 + 1, 68 + 17, 68 + 25, 68 + 29, 68 + 31, 68 + 32, 68 + 33] and out == 68


def test_ring_rule_rejects_what_window_index_table_rejects():
    for bad in [(1, 2, 3), (0, 3, 2), (0, 0, 1), ()]:
        with pytest.raises(ValueError, match="skip_length"):
            window_index_table(4, bad)
        with pytest.raises(ValueError, match="skip_length"):
            stream_window_row(4, 0, bad)
    with pytest.raises(ValueError):
        stream_window_row(-1, 0)


@pytest.fixture(scope="module")
def lib():
    from coupe.dvsg_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.dvsg_last_error_string()


def test_inplace_ring_rejects_bad_arguments(lib):
    f = lib.dvsg_stabilize_ring_inplace_f32
    #          net pr pool n_pool table slots  B  H  W   F  xs ys ws nbytes stream
    assert f(None, 0, 8, 34, 8, 8, 1, 8, 8, 8, None, None, 8, 1 << 20, None) == -1
    assert b"NULL" in _err(lib)
    assert f(8, 0, 8, 34, 8, None, 1, 8, 8, 8, None, None, 8, 1 << 20, None) == -1
    assert b"out_slots" in _err(lib)
    assert f(8, 0, None, 34, 8, 8, 1, 8, 8, 8, None, None, 8, 1 << 20, None) == -1
    assert b"NULL" in _err(lib)
    assert f(8, 0, 8, 34, 8, 8, 0, 8, 8, 8, None, None, 8, 1 << 20, None) == -1
    assert b"B=0" in _err(lib)
    assert f(8, 0, 8, 0, 8, 8, 1, 8, 8, 8, None, None, 8, 1 << 20, None) == -1
    assert b"n_pool=0" in _err(lib)
    assert f(8, 9, 8, 34, 8, 8, 1, 8, 8, 8, None, None, 8, 1 << 20, None) == -1
    assert b"unknown precision" in _err(lib)


def test_ingest_rejects_bad_arguments(lib):
    f = lib.dvsg_frames_ingest_u8
    #          src n sH sW flip pool n_pool slots dH dW u8 u8W u8x0 stream
    assert f(None, 1, 8, 8, 0, 8, 4, 8, 8, 8, None, 0, 0, None) == -1
    assert b"NULL" in _err(lib)
    assert f(8, 1, 8, 8, 0, 8, 4, None, 8, 8, None, 0, 0, None) == -1
    assert b"NULL" in _err(lib)
    assert f(8, 0, 8, 8, 0, 8, 4, 8, 8, 8, None, 0, 0, None) == -1
    assert b"bad shape" in _err(lib)
    assert f(8, 1, 8, 8, 0, 8, 0, 8, 8, 8, None, 0, 0, None) == -1
    assert b"bad shape" in _err(lib)
    assert f(8, 1, 8, 0, 0, 8, 4, 8, 8, 8, None, 0, 0, None) == -1
    assert b"bad shape" in _err(lib)
    assert f(8, 1, 8, 8, 0, 8, 4, 8, 8, 8, 8, 16, 0, None) == -1      # same size: the u8 half comes from the pool
    assert b"uint8 half" in _err(lib)
    assert f(8, 1, 16, 16, 0, 8, 4, 8, 8, 8, 8, 12, 8, None) == -1    # resized: columns [8,16) do not fit 12
    assert b"do not fit" in _err(lib)


def test_f32_to_u8_slots_rejects_bad_arguments(lib):
    f = lib.dvsg_frames_f32_to_u8_slots
    #          pool n_pool slots n H W flip dst dstW x0 stream
    assert f(None, 4, 8, 1, 8, 8, 0, 8, 8, 0, None) == -1
    assert b"NULL" in _err(lib)
    assert f(8, 4, None, 1, 8, 8, 0, 8, 8, 0, None) == -1
    assert b"NULL" in _err(lib)
    assert f(8, 4, 8, 1, 8, 8, 0, None, 8, 0, None) == -1
    assert b"NULL" in _err(lib)
    assert f(8, 4, 8, 0, 8, 8, 0, 8, 8, 0, None) == -1
    assert b"bad shape" in _err(lib)
    assert f(8, 0, 8, 1, 8, 8, 0, 8, 8, 0, None) == -1
    assert b"n_pool=0" in _err(lib)
    assert f(8, 4, 8, 1, 8, 8, 0, 8, 16, 9, None) == -1
    assert b"do not fit" in _err(lib)
