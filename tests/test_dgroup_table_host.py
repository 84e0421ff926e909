"""CPU-only: the layout and the argument rules of data groups over a table of streams (vit_data_groups_table_layout,
include/viterbi_amd.h) against a few lines of numpy.  tests/test_gpu_dgroup_table.py takes layout_model from here."""
import numpy as np
import pytest

SLOT = 24
MAX_STREAMS = 64
MAX_SLOTS, MAX_TABLE_SLOTS = 1 << 24, 1 << 26


def layout_model(rows):
    """(offset, rec_index, nslots, max_groups, data_capacity, records_only) rows ->
    (dg_index, data_offset, ndg, data_bytes, bytes_end, rec_end)"""
    t = np.array([[int(v) for v in r] for r in rows], dtype=object).reshape(-1, 6)
    offset, rec_index, nslots, max_groups, cap = (t[:, j] for j in range(5))
    rounded = (cap + 15) // 16 * 16
    dg_index = [int(v) for v in np.cumsum(max_groups) - max_groups]
    data_offset = [int(v) for v in np.cumsum(rounded) - rounded]
    return (dg_index, data_offset, int(max_groups.sum()), int(rounded.sum()), int((offset + SLOT * nslots).max()),
            int((rec_index + nslots).max()))


def check_layout(V, rows):
    lay = V.data_groups_table_layout(np.array(rows, V.DG_STREAM_DTYPE))
    dg_index, data_offset, ndg, data_bytes, bytes_end, rec_end = layout_model(rows)
    n = len(rows)
    assert lay["dg_index"][:n].tolist() == dg_index and lay["data_offset"][:n].tolist() == data_offset
    assert not lay["dg_index"][n:].any() and not lay["data_offset"][n:].any()
    assert (int(lay["ndg"]), int(lay["data_bytes"]), int(lay["bytes_end"]), int(lay["rec_end"])) == (ndg, data_bytes, bytes_end, rec_end)
    return lay


def random_rows(rng, n):
    rows = []
    for _ in range(n):
        ro = int(rng.integers(0, 4) == 0)
        rows.append((int(rng.integers(0, 1 << 20)), int(rng.integers(0, 1 << 20)), int(rng.integers(1, 5000)),
                     int(rng.integers(0, 300)) * int(rng.integers(0, 4) != 0), 0 if ro else int(rng.integers(0, 70000)), ro))
    return rows


# ---- the binding ----------------------------------------------------------------------------------------------------------
def test_exported_and_bound(V):
    assert {"vit_data_groups_table_layout", "vit_data_groups_table_dev"} <= set(V.EXPORTS)
    assert hasattr(V.lib(), "vit_data_groups_table_layout") and hasattr(V.lib(), "vit_data_groups_table_dev")
    assert callable(V.data_groups_table_layout) and callable(V.data_groups_table_dev)
    assert V.DG_STREAM_DTYPE.itemsize == 32 and V.DG_LAYOUT_DTYPE.itemsize == 8 * (2 * MAX_STREAMS + 4)
    assert V.DG_MAX_STREAMS == MAX_STREAMS == V.PKT_MAX_STREAMS
    assert V.DG_STREAM_DTYPE.names == ("offset", "rec_index", "nslots", "max_groups", "data_capacity", "records_only")


# ---- layout ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 64])
def test_layout_of_random_tables(V, n):
    rng = np.random.default_rng(100 + n)
    for _ in range(20):
        check_layout(V, random_rows(rng, n))


def test_layout_rounds_each_capacity_to_16(V):
    caps = [0, 1, 15, 16, 17, 0, 33]
    lay = check_layout(V, [(100 * k, 7 * k, 10 + k, 3, c, 0) for k, c in enumerate(caps)])
    assert lay["data_offset"][:7].tolist() == [0, 0, 16, 32, 48, 80, 80] and int(lay["data_bytes"]) == 128


def test_layout_max_groups_0_and_records_only(V):
    lay = check_layout(V, [(0, 0, 5, 0, 40, 0), (0, 0, 5, 4, 0, 1), (7, 1, 9, 0, 0, 1), (0, 0, 5, 2, 16, 0)])
    assert lay["dg_index"][:4].tolist() == [0, 0, 4, 4] and int(lay["ndg"]) == 6
    assert lay["data_offset"][:4].tolist() == [0, 48, 48, 48] and int(lay["data_bytes"]) == 64


def test_layout_takes_overlapping_and_repeated_streams(V):
    """the input is only read: bytes_end and rec_end are maxima, not sums"""
    lay = check_layout(V, [(1000, 50, 100, 1, 0, 0), (1000, 50, 100, 1, 0, 0), (1024, 51, 10, 1, 0, 0), (0, 900, 3, 1, 0, 0)])
    assert (int(lay["bytes_end"]), int(lay["rec_end"])) == (1000 + 2400, 903)


def test_layout_at_the_caps(V):
    check_layout(V, [(0, 0, MAX_SLOTS, 0, 0, 1)] * 4)                                       # 1<<26 slots in all
    check_layout(V, [((1 << 64) - 1 - SLOT, (1 << 64) - 2, 1, 0, 0, 1)])                    # the ends just fit 64 bits
    lay = check_layout(V, [(0, 0, 1, 0xFFFFFFFF, 0xFFFFFFF0, 0), (0, 0, 1, 5, 16, 0)])      # the second entry starts below 2^32
    assert lay["dg_index"][1] == 0xFFFFFFFF and lay["data_offset"][1] == 0xFFFFFFF0


# ---- rejections -----------------------------------------------------------------------------------------------------------
GOOD = (100, 7, 50, 4, 100, 0)


def rejected(V, rows, n=None, text=None):
    tab = np.array(rows, V.DG_STREAM_DTYPE).reshape(-1)
    out = np.full(V.DG_LAYOUT_DTYPE.itemsize, 0x77, np.uint8)
    rc = V.lib().vit_data_groups_table_layout(tab.ctypes.data, len(tab) if n is None else n, out.ctypes.data)
    assert rc == 1, rows  # VIT_ERR_ARG
    assert (out == 0x77).all(), "a rejected table writes no layout"
    assert "vit_data_groups_table_layout" in V.last_error()
    if text:
        assert text in V.last_error(), V.last_error()
    if n is None:
        with pytest.raises(V.ViterbiError):
            V.data_groups_table_layout(tab)


def test_layout_rejections(V):
    V.data_groups_table_layout(np.array([GOOD], V.DG_STREAM_DTYPE))
    rejected(V, [GOOD], n=0, text="nstreams")
    rejected(V, [GOOD] * 65, n=65, text="nstreams")
    o, r, ns, mg, cap, ro = GOOD
    rejected(V, [(o, r, 0, mg, cap, ro)], text="entry 0")
    rejected(V, [GOOD, GOOD, (o, r, MAX_SLOTS + 1, mg, cap, ro)], text="entry 2")
    V.data_groups_table_layout(np.array([(o, r, MAX_SLOTS, mg, cap, ro)], V.DG_STREAM_DTYPE))
    rejected(V, [GOOD, (o, r, ns, mg, 0, 2)], text="entry 1")
    rejected(V, [(o, r, ns, mg, 1, 1)], text="entry 0")
    V.data_groups_table_layout(np.array([(o, r, ns, mg, 0, 1)], V.DG_STREAM_DTYPE))
    rejected(V, [GOOD, ((1 << 64) - SLOT, r, 1, mg, cap, ro)], text="entry 1")          # offset + 24*nslots
    rejected(V, [((1 << 64) - 24 * 50 + 1, r, 50, mg, cap, ro)], text="entry 0")
    rejected(V, [GOOD] * 5 + [(o, (1 << 64) - 50, 50, mg, cap, ro)], text="entry 5")      # rec_index + nslots
    rejected(V, [(o, (1 << 64) - 1, 1, mg, cap, ro)], text="entry 0")
    # a NULL table or layout
    assert V.lib().vit_data_groups_table_layout(None, 1, np.zeros(2000, np.uint8).ctypes.data) == 1
    assert V.lib().vit_data_groups_table_layout(np.array([GOOD], V.DG_STREAM_DTYPE).ctypes.data, 1, None) == 1
    assert "vit_data_groups_table_layout" in V.last_error()


def test_layout_rejects_more_than_2_26_slots(V):
    big = (0, 0, MAX_SLOTS, 0, 0, 1)
    rejected(V, [big] * 4 + [(0, 0, 1, 0, 0, 1)], text="entry 4")
    rejected(V, [big, GOOD, big, big, big], text="entry 4")
    assert "1<<26" in V.last_error()


def test_layout_rejects_an_index_past_2_32(V):
    rejected(V, [(0, 0, 1, 0xFFFFFFFF, 0, 0), (0, 0, 1, 1, 0, 0), (0, 0, 1, 0, 0, 0)], text="entry 2")
    assert "dg_index" in V.last_error()
    rejected(V, [(0, 0, 1, 0, 0xFFFFFFF1, 0), (0, 0, 1, 0, 0, 0)], text="entry 1")
    assert "data_offset" in V.last_error()
    V.data_groups_table_layout(np.array([(0, 0, 1, 0, 0xFFFFFFF1, 0)], V.DG_STREAM_DTYPE))     # the sizes themselves may pass it
