"""CPU-only: the layout and the argument rules of packet mode over a table of streams (vit_packet_table_layout,
include/viterbi_amd.h) against a few lines of Python, and the model of the phase pick that tests/test_gpu_packet_table.py
compares the device with."""
import numpy as np
import pytest

SLOT, FEC_SLOTS = 24, 103
FEC_NONE, FEC_PHASE, FEC_SEARCH = 0, 1, 2
NO_PHASE = 0xFFFFFFFF
MAX_STREAMS = 64


# ---- models -------------------------------------------------------------------------------------------------------------
def layout_model(tab):
    """(offset, framebytes, nframes, ...) rows -> (rec_index, fec_index, nrec, nfecrec, bytes_end)"""
    rec_index, fec_index, nrec, nfecrec, end = [], [], 0, 0, 0
    for row in tab:
        offset, framebytes, nframes = int(row[0]), int(row[1]), int(row[2])
        nslots = nframes * framebytes // SLOT
        rec_index.append(nrec)
        fec_index.append(nfecrec)
        nrec += nslots
        nfecrec += nslots // FEC_SLOTS
        end = max(end, offset + SLOT * nslots)
    return rec_index, fec_index, nrec, nfecrec, end


def fec_count(nslots, phase):
    return (nslots - phase) // FEC_SLOTS if nslots > phase else 0


def pick_model(scores, min_score):
    """the 103 scores of a FEC_SEARCH stream -> (phase or NO_PHASE, score, runner_up): the largest score, the SMALLEST
    phase that has it, the largest score at any other phase; no phase unless score >= max(min_score, 1)"""
    scores = [int(x) for x in scores]
    assert len(scores) == FEC_SLOTS
    score = max(scores)
    p = scores.index(score)
    runner_up = max(scores[:p] + scores[p + 1:])
    return (p if score >= max(int(min_score), 1) else NO_PHASE), score, runner_up


def stream_rec_model(fec, phase, min_score, nslots, scores):
    """a table entry and its stream's scores -> (phase, score, runner_up, nfec) of its vit_pkt_stream_rec"""
    if fec == FEC_NONE:
        return NO_PHASE, 0, 0, 0
    if fec == FEC_PHASE:
        return phase, 0, 0, fec_count(nslots, phase)
    p, score, runner_up = pick_model(scores, min_score)
    return p, score, runner_up, 0 if p == NO_PHASE else fec_count(nslots, p)


def random_table(rng, n, gap=lambda rng: int(rng.integers(0, 40))):
    rows, offset = [], int(rng.integers(0, 100))
    for _ in range(n):
        framebytes = SLOT * int(rng.integers(1, 49))
        nframes = int(rng.integers(1, 400))
        fec = int(rng.integers(0, 3))
        rows.append((offset, framebytes, nframes, fec, int(rng.integers(0, FEC_SLOTS)) if fec == FEC_PHASE else 0,
                     int(rng.integers(0, 50)) if fec == FEC_SEARCH else 0, 0))
        offset += framebytes * nframes + gap(rng)
    order = rng.permutation(n)  # table order is not address order
    return [rows[k] for k in order]


def check_layout(V, rows):
    lay = V.packet_table_layout(np.array(rows, V.PKT_STREAM_DTYPE))
    rec_index, fec_index, nrec, nfecrec, end = layout_model(rows)
    n = len(rows)
    assert lay["rec_index"][:n].tolist() == rec_index and lay["fec_index"][:n].tolist() == fec_index
    assert not lay["rec_index"][n:].any() and not lay["fec_index"][n:].any()
    assert (int(lay["nrec"]), int(lay["nfecrec"]), int(lay["bytes_end"])) == (nrec, nfecrec, end)
    return lay


# ---- the binding ----------------------------------------------------------------------------------------------------------
def test_record_sizes(V):
    assert V.PKT_STREAM_DTYPE.itemsize == 32 and V.PKT_STREAM_REC_DTYPE.itemsize == 16
    assert V.PKT_LAYOUT_DTYPE.itemsize == 8 * (2 * MAX_STREAMS + 3)
    assert (V.PKT_MAX_STREAMS, V.PKT_FEC_NONE, V.PKT_FEC_PHASE, V.PKT_FEC_SEARCH, V.PKT_NO_PHASE) == (64, 0, 1, 2, NO_PHASE)
    assert V.PKT_MAX_STREAMS == V.ENS_MAX_SUBCH


# ---- layout ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 64])
def test_layout_of_random_tables(V, n):
    rng = np.random.default_rng(n)
    for _ in range(20):
        check_layout(V, random_table(rng, n))
    # streams that touch: the end of one is the start of the next
    check_layout(V, random_table(rng, n, gap=lambda rng: 0))


def test_layout_small_and_large_entries(V):
    # fewer slots than an FEC frame reserve no FEC record; 103 slots reserve one whatever the mode
    lay = check_layout(V, [(0, 24, 102, FEC_SEARCH, 0, 0, 0), (5000, 24, 103, FEC_NONE, 0, 0, 0), (10000, 1152, 3, FEC_PHASE, 102, 0, 0)])
    assert lay["fec_index"][:3].tolist() == [0, 0, 1] and int(lay["nfecrec"]) == 2
    # 2^31 slots in all are still taken, offsets beyond 2^32 too
    big = 1 << 25
    lay = check_layout(V, [(0, 1152, big, 0, 0, 0, 0), (1 << 40, 384, big, 0, 0, 0, 0)])
    assert int(lay["nrec"]) == 1 << 31 and int(lay["bytes_end"]) == (1 << 40) + 384 * big


def test_layout_from_ensemble_offsets(V):
    """the recipe of INTEGRATION.md 2m-2: the RSDims 0 entries of a sub-channel table, each at its work_offset"""
    sub = np.zeros(5, V.ENS_SUBCH_DTYPE)
    sub["framebits"] = [192 * 8, 1536, 192 * 3, 9216, 192]
    sub["RSDims"] = [8, 0, 3, 0, 0]
    sub["nframes"] = [10, 200, 5, 7, 120]
    ens = V.ensemble_layout(sub)
    packet = [k for k in range(5) if sub["RSDims"][k] == 0]
    rows = [(int(ens["work_offset"][k]), int(sub["framebits"][k]) // 8, int(sub["nframes"][k]), FEC_SEARCH, 0, 0, 0) for k in packet]
    lay = check_layout(V, rows)
    slots = [200 * 8, 7 * 48, 120]
    assert lay["rec_index"][:3].tolist() == [0, slots[0], slots[0] + slots[1]]
    assert lay["fec_index"][:3].tolist() == [0, 15, 18] and int(lay["nfecrec"]) == 19
    assert int(lay["bytes_end"]) == int(ens["work_bytes"])  # the last entry is a packet-mode one


# ---- rejections -----------------------------------------------------------------------------------------------------------
GOOD = (100, 192, 50, FEC_SEARCH, 0, 5, 0)


def rejected(V, rows, n=None, text=None):
    tab = np.array(rows, V.PKT_STREAM_DTYPE).reshape(-1)
    out = np.full(1, 0x77, np.uint8).repeat(V.PKT_LAYOUT_DTYPE.itemsize)
    rc = V.lib().vit_packet_table_layout(tab.ctypes.data, len(tab) if n is None else n, out.ctypes.data)
    assert rc == 1, rows  # VIT_ERR_ARG
    assert (out == 0x77).all(), "a rejected table writes no layout"
    assert "vit_packet_table_layout" in V.last_error()
    if text:
        assert text in V.last_error(), V.last_error()
    if n is None:
        with pytest.raises(V.ViterbiError):
            V.packet_table_layout(tab)


def test_layout_rejections(V):
    V.packet_table_layout(np.array([GOOD], V.PKT_STREAM_DTYPE))
    rejected(V, [GOOD], n=0)
    rejected(V, [GOOD] * 65, n=65)
    o, fb, nf, fec, ph, ms, rs = GOOD
    for framebytes in (0, 23, 25, 1152 + 24, 1153, 12):
        rejected(V, [(o, framebytes, nf, fec, ph, ms, rs)], text="entry 0")
    rejected(V, [GOOD, (10 ** 6, fb, 0, fec, ph, ms, rs)], text="entry 1")
    rejected(V, [(o, fb, nf, 3, 0, 0, 0)], text="entry 0")
    rejected(V, [(o, fb, nf, FEC_PHASE, 103, 0, 0)], text="entry 0")
    rejected(V, [(o, fb, nf, FEC_NONE, 1, 0, 0)], text="phase")
    rejected(V, [(o, fb, nf, FEC_SEARCH, 1, 0, 0)], text="phase")
    rejected(V, [(o, fb, nf, FEC_NONE, 0, 1, 0)], text="min_score")
    rejected(V, [(o, fb, nf, FEC_PHASE, 5, 1, 0)], text="min_score")
    rejected(V, [(o, fb, nf, fec, ph, ms, 1)], text="reserved")
    V.packet_table_layout(np.array([(o, fb, nf, FEC_PHASE, 102, 0, 0)], V.PKT_STREAM_DTYPE))
    # a NULL table or layout
    assert V.lib().vit_packet_table_layout(None, 1, np.zeros(2000, np.uint8).ctypes.data) == 1
    assert V.lib().vit_packet_table_layout(np.array([GOOD], V.PKT_STREAM_DTYPE).ctypes.data, 1, None) == 1


def test_layout_rejects_overlapping_streams(V):
    n = 192 * 50
    V.packet_table_layout(np.array([GOOD, (100 + n, 24, 1, 0, 0, 0, 0)], V.PKT_STREAM_DTYPE))  # touching
    rejected(V, [GOOD, (100 + n - 1, 24, 1, 0, 0, 0, 0)], text="overlap")
    rejected(V, [(100 + n - 1, 24, 1, 0, 0, 0, 0), GOOD], text="overlap")  # in either table order
    rejected(V, [GOOD, GOOD], text="overlap")
    rejected(V, [GOOD, (0, 24, 5, 0, 0, 0, 0)], text="overlap")  # bytes 0 ... 119 reach into 100 ...
    rejected(V, [(0, 24, 4, 0, 0, 0, 0), GOOD, (10 ** 5, 24, 9, 0, 0, 0, 0), (200, 48, 1, 0, 0, 0, 0)], text="overlap")  # 1 and 3
    # a stream whose end does not fit 64 bits
    rejected(V, [((1 << 64) - 24, 24, 1, 0, 0, 0, 0)], text="entry 0")
    V.packet_table_layout(np.array([((1 << 64) - 25, 24, 1, 0, 0, 0, 0)], V.PKT_STREAM_DTYPE))


def test_layout_rejects_more_than_2_31_slots(V):
    big = 1 << 25
    rejected(V, [(0, 1152, big, 0, 0, 0, 0), (1 << 40, 384, big, 0, 0, 0, 0), (1 << 41, 24, 1, 0, 0, 0, 0)], text="entry 2")
    rejected(V, [(k << 40, 1152, (1 << 32) - 1, 0, 0, 0, 0) for k in range(64)])


# ---- the pick -------------------------------------------------------------------------------------------------------------
def test_pick_model():
    z = [0] * FEC_SLOTS
    assert pick_model(z, 0) == (NO_PHASE, 0, 0) and pick_model(z, 7) == (NO_PHASE, 0, 0)
    one = z.copy()
    one[102] = 1
    assert pick_model(one, 0) == (102, 1, 0) and pick_model(one, 1) == (102, 1, 0)  # min_score 0 means "at least 1"
    assert pick_model(one, 2) == (NO_PHASE, 1, 0)
    tie = z.copy()
    tie[64], tie[17], tie[3] = 27, 27, 26
    assert pick_model(tie, 0) == (17, 27, 27) and pick_model(tie, 27) == (17, 27, 27) and pick_model(tie, 28) == (NO_PHASE, 27, 27)
    tie[0] = 27
    assert pick_model(tie, 0) == (0, 27, 27)
    clear = z.copy()
    clear[63], clear[64], clear[65] = 8, 9, 7
    assert pick_model(clear, 9) == (64, 9, 8) and pick_model(clear, 10) == (NO_PHASE, 9, 8)
    assert pick_model([5] * FEC_SLOTS, 0) == (0, 5, 5)
    rng = np.random.default_rng(0)
    for _ in range(50):
        s = rng.integers(0, 4, FEC_SLOTS)
        p, score, ru = pick_model(s, 2)
        assert score == s.max() and (p == NO_PHASE) == (score < 2)
        if p != NO_PHASE:
            assert s[p] == score and (s[:p] < score).all() and ru == np.delete(s, p).max()


def test_stream_rec_model():
    s = [0] * FEC_SLOTS
    s[1] = 9
    assert stream_rec_model(FEC_NONE, 0, 0, 500, s) == (NO_PHASE, 0, 0, 0)
    assert stream_rec_model(FEC_PHASE, 102, 0, 205, s) == (102, 0, 0, 1) and stream_rec_model(FEC_PHASE, 5, 0, 5, s) == (5, 0, 0, 0)
    assert stream_rec_model(FEC_SEARCH, 0, 0, 207, s) == (1, 9, 0, 2) and stream_rec_model(FEC_SEARCH, 0, 10, 207, s) == (NO_PHASE, 9, 0, 0)
