"""Host: the layout of a whole ensemble's sub-channel table (vit_ensemble_layout, include/viterbi_amd.h) against a numpy
restatement of the rule, and every table the call rejects.  Needs no GPU."""
import ctypes as C

import numpy as np
import pytest

MAX_SUBCH = 64


def entry(framebits=None, rsdims=0, nframes=None, phase=0, col=0, profile=0, nsym=0, reserved=0):
    """one table entry as a tuple in ENS_SUBCH_DTYPE's order; DAB+ defaults: framebits 192*rsdims, one superframe"""
    if framebits is None:
        framebits = 192 * rsdims
    if nframes is None:
        nframes = 5 if rsdims else 1
    return (col, profile, framebits, rsdims, phase, nframes, nsym, reserved)


def layout_model(sub):
    """the layout rule: blocks in table order, each at the next multiple of 16 bytes; one record per DAB+ superframe"""
    fb, rs, nf = (sub[k].astype(np.int64) for k in ("framebits", "RSDims", "nframes"))
    work_len, rs_len, recs = nf * (fb // 8), np.where(rs > 0, nf // 5 * 110 * rs, 0), np.where(rs > 0, nf // 5, 0)
    wo, ro, w, r = [], [], 0, 0
    for k in range(len(sub)):
        wo.append(-(-w // 16) * 16)
        ro.append(-(-r // 16) * 16)
        w, r = wo[k] + int(work_len[k]), ro[k] + int(rs_len[k])
    rec = np.concatenate(([0], np.cumsum(recs)))
    return dict(work_offset=wo, rs_offset=ro, rec_index=rec[:-1].tolist(), work_bytes=w, rs_bytes=r, nrec=int(rec[-1]),
                rows_needed=int((sub["phase"].astype(np.int64) + nf).max()) + 15, max_framebits=int(fb.max()))


def random_table(rng, nsub):
    rows = []
    for _ in range(nsub):
        if rng.random() < 0.75:
            rows.append(entry(rsdims=int(rng.integers(1, 49)), nframes=5 * int(rng.integers(1, 40)),
                              phase=int(rng.integers(0, 30)), col=64 * int(rng.integers(0, 800))))
        else:
            rows.append(entry(framebits=8 * int(rng.integers(1, 1153)), nframes=int(rng.integers(1, 200)),
                              phase=int(rng.integers(0, 30))))
    return rows


def check(V, rows):
    sub = np.array(rows, V.ENS_SUBCH_DTYPE)
    got, want = V.ensemble_layout(sub), layout_model(sub)
    n = len(rows)
    for k in ("work_offset", "rs_offset", "rec_index"):
        assert got[k][:n].tolist() == want[k], k
        assert not got[k][n:].any(), k  # entries behind the table: 0
    for k in ("work_bytes", "rs_bytes", "nrec", "rows_needed", "max_framebits"):
        assert int(got[k]) == want[k], k
    return got


def test_struct_sizes(V):
    assert V.ENS_SUBCH_DTYPE.itemsize == 32
    assert V.ENS_LAYOUT_DTYPE.itemsize == 3 * 8 * MAX_SUBCH + 3 * 8 + 2 * 4


def test_random_tables_against_the_rule(V):
    rng = np.random.default_rng(1)
    for nsub in [1, 2, 3, 17, 63, 64] + [int(x) for x in rng.integers(1, 65, 40)]:
        check(V, random_table(rng, nsub))


def test_odd_rsdims_start_on_16_byte_boundaries(V):
    """RSDims 1, 3, 7: blocks of 360/330, 360/330 and 1680/1540 bytes, whose ends are mostly no multiples of 16"""
    got = check(V, [entry(rsdims=1, nframes=15), entry(rsdims=3), entry(rsdims=7, nframes=10), entry(rsdims=5)])
    assert got["work_offset"][:4].tolist() == [0, 368, 368 + 368, 736 + 1680]
    assert got["rs_offset"][:4].tolist() == [0, 336, 336 + 336, 672 + 1552]
    assert got["rec_index"][:4].tolist() == [0, 3, 4, 6] and got["nrec"] == 7
    assert all(o % 16 == 0 for o in got["work_offset"].tolist() + got["rs_offset"].tolist())


def test_not_dabplus_takes_nothing_in_rs_out_and_no_record(V):
    got = check(V, [entry(rsdims=3), entry(framebits=1536, nframes=3), entry(framebits=8), entry(rsdims=2, nframes=10)])
    assert got["rs_offset"][:4].tolist() == [0, 336, 336, 336] and got["rs_bytes"] == 336 + 2 * 220
    assert got["rec_index"][:4].tolist() == [0, 1, 1, 1] and got["nrec"] == 3
    assert got["work_offset"][:4].tolist() == [0, 368, 368 + 576, 960] and got["work_bytes"] == 960 + 480


def test_rows_needed_and_max_framebits(V):
    got = check(V, [entry(rsdims=48, phase=0, nframes=5), entry(rsdims=1, phase=7, nframes=10), entry(framebits=9216, phase=3)])
    assert got["rows_needed"] == 7 + 10 + 15 and got["max_framebits"] == 9216
    assert check(V, [entry(framebits=8)])["rows_needed"] == 16


def test_nsub_1_and_64(V):
    check(V, [entry(rsdims=48, nframes=500)])
    got = check(V, [entry(rsdims=1 + k % 48, phase=k % 5) for k in range(MAX_SUBCH)])
    assert got["nrec"] == MAX_SUBCH


BAD = {
    "framebits 0": entry(framebits=0),
    "framebits no multiple of 8": entry(framebits=772),
    "framebits even, no multiple of 8": entry(framebits=770),
    "framebits above 9216": entry(framebits=9224),
    "RSDims 49": entry(framebits=9216, rsdims=49),
    "RSDims 49 with its own framebits": entry(rsdims=49),
    "DAB+ framebits not 192*RSDims": entry(framebits=192 * 4, rsdims=5),
    "DAB+ nframes no multiple of 5": entry(rsdims=4, nframes=12),
    "nframes 0": entry(framebits=768, nframes=0),
    "DAB+ nframes 0": entry(rsdims=4, nframes=0),
    "reserved": entry(rsdims=4, reserved=1),
}


@pytest.mark.parametrize("what", sorted(BAD))
@pytest.mark.parametrize("at", [0, 5])
def test_rejected_tables(V, what, at):
    """each broken rule alone, in the first and in a later entry: VIT_ERR_ARG, and the error text names the entry"""
    rows = [entry(rsdims=2 + k) for k in range(7)]
    rows[at] = BAD[what]
    sub = np.array(rows, V.ENS_SUBCH_DTYPE)
    out = np.zeros(1, V.ENS_LAYOUT_DTYPE)
    assert V.lib().vit_ensemble_layout(sub.ctypes.data_as(C.c_void_p), len(rows), out.ctypes.data_as(C.c_void_p)) == 1
    msg = V.last_error()
    assert msg and "vit_ensemble_layout" in msg and "entry %d" % at in msg, msg
    with pytest.raises(V.ViterbiError):
        V.ensemble_layout(sub)


@pytest.mark.parametrize("nsub", [0, 65, 1 << 31])
def test_rejected_nsub(V, nsub):
    sub = np.array([entry(rsdims=2)] * 65, V.ENS_SUBCH_DTYPE)
    out = np.zeros(1, V.ENS_LAYOUT_DTYPE)
    assert V.lib().vit_ensemble_layout(sub.ctypes.data_as(C.c_void_p), nsub, out.ctypes.data_as(C.c_void_p)) == 1
    assert "nsub" in V.last_error()
    assert V.lib().vit_ensemble_layout(None, 1, out.ctypes.data_as(C.c_void_p)) == 1 and V.last_error()
    assert V.lib().vit_ensemble_layout(sub.ctypes.data_as(C.c_void_p), 1, None) == 1 and V.last_error()


def test_device_entry_points_validate_first_or_report_no_device(V):
    """the table calls run the same validation: without a device VIT_ERR_NO_DEVICE, with one VIT_ERR_ARG; nothing is
    launched either way"""
    import torch
    want = 1 if torch.cuda.is_available() else 2
    sub = np.array([entry(rsdims=4, nframes=12)], V.ENS_SUBCH_DTYPE)
    p = sub.ctypes.data_as(C.c_void_p)
    assert V.lib().vit_rs_table_dev(None, None, None, p, 1, None) == want
    assert V.lib().vit_dabplus_aus_table_dev(None, 0, p, 1, None, None, None) == want
    assert V.lib().vit_ensemble_dev(None, 0, p, 1, None, 0, 128, None, None, None, None, None, None) == want
    assert V.last_error()
