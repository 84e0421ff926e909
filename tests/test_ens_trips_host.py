"""Host: the pass geometry of the table RS kernel (rs_table_kernel, csrc/rs_table.hip) restated in numpy, and the tables
from which tests/test_gpu_ens_trips.py drives that kernel past its first loop trip.  Needs no GPU.

rs_table_launch starts min(npass, 4 * CUs) workgroups; workgroup b takes passes b, b + grid, b + 2 grid, ...  A pass
belongs to ONE sub-channel and holds 256 // RSDims of its superframes.  `passes` states that rule pass by pass,
`trip_facts` counts what a table makes the workgroups do, and the tests below prove that the generated table meets every
precondition the GPU test asserts - for the CU counts of the devices this runs on (256; 304 and 8 as other sizes), so a
GPU test that cannot reach a later trip fails here first."""
import math
import os
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import reffix  # noqa: E402
import rsdirect as D  # noqa: E402
from test_gpu_ensemble import table  # noqa: E402  (a helper only: nothing here touches a GPU)

MAX_SUBCH = 64
RS_THREADS = 256


def dab(r, nsf):
    return (192 * r, r, 5 * nsf)


def plain(bits, nframes):
    """an entry that is not DAB+: no record, no RS pass, nothing in d_rs_out"""
    return (bits, 0, nframes)


# ---- the mirror -----------------------------------------------------------------------------------------------------

def passes(rows, cus, lay):
    """rows as for `table`, lay = V.ensemble_layout of them -> the launch of rs_table_kernel on a device of `cus` CUs:
    per pass g its sub-channel, rsdims, sf0 (first superframe within the sub-channel), nloc, first record, input and
    output offset; the grid; and per workgroup the list of its passes (its trips).  Built by walking the table in order,
    every offset by accumulation from the layout's block starts."""
    sub, rsdims, sf0, nloc, rec, in_off, out_off, pass0 = [], [], [], [], [], [], [], []
    for k, row in enumerate(rows):
        r, nsf = int(row[1]), int(row[2]) // 5 if row[1] else 0
        pass0.append(len(sub))
        if not r:
            continue
        spb = RS_THREADS // r
        i, o, q, s = int(lay["work_offset"][k]), int(lay["rs_offset"][k]), int(lay["rec_index"][k]), 0
        while s < nsf:
            n = min(spb, nsf - s)
            sub.append(k), rsdims.append(r), sf0.append(s), nloc.append(n), rec.append(q), in_off.append(i), out_off.append(o)
            i, o, q, s = i + n * 120 * r, o + n * 110 * r, q + n, s + n
    m = types.SimpleNamespace(**{n: np.array(v, np.int64) for n, v in (
        ("sub", sub), ("rsdims", rsdims), ("sf0", sf0), ("nloc", nloc), ("rec", rec), ("in_off", in_off), ("out_off", out_off),
        ("pass0", pass0))})
    m.npass = len(sub)
    m.grid = min(m.npass, 4 * cus)
    m.trips = [list(range(b, m.npass, m.grid)) for b in range(m.grid)]
    m.trip_of = np.arange(m.npass) // max(m.grid, 1)  # pass g is trip g // grid of workgroup g % grid
    m.spb = RS_THREADS // np.maximum(m.rsdims, 1)
    return m


def find(starts, x):
    """vit_ens_find (csrc/vit_internal.h): the largest k whose start is <= x"""
    return np.searchsorted(np.asarray(starts), x, side="right") - 1


def check_mirror(V, rows, cus):
    sub = table(V, rows)
    lay = V.ensemble_layout(sub)
    m = passes(rows, cus, lay)
    r = np.array([row[1] for row in rows], np.int64)
    nsf = np.where(r > 0, np.array([row[2] for row in rows], np.int64) // 5, 0)
    nrec = int(lay["nrec"])
    assert nrec == nsf.sum() and m.npass == int((-(-nsf // (RS_THREADS // np.maximum(r, 1))))[r > 0].sum())
    assert m.grid == min(m.npass, 4 * cus) and sorted(g for t in m.trips for g in t) == list(range(m.npass))
    assert all(t == list(range(t[0], m.npass, m.grid)) for t in m.trips)
    # every record exactly once and in order
    covered = np.concatenate([np.arange(q, q + n) for q, n in zip(m.rec, m.nloc)]) if m.npass else np.zeros(0, np.int64)
    assert np.array_equal(covered, np.arange(nrec))
    assert (m.nloc >= 1).all() and (m.nloc <= m.spb).all() and (m.sf0 % m.spb == 0).all()
    # the kernel's closed forms
    wo, ro, ri = (lay[n][:len(rows)].astype(np.int64) for n in ("work_offset", "rs_offset", "rec_index"))
    assert np.array_equal(m.rsdims, r[m.sub]) and (m.rsdims > 0).all()
    assert np.array_equal(m.in_off, wo[m.sub] + m.sf0 * 120 * m.rsdims)
    assert np.array_equal(m.out_off, ro[m.sub] + m.sf0 * 110 * m.rsdims)
    assert np.array_equal(m.rec, ri[m.sub] + m.sf0)
    assert np.array_equal(m.sf0, (np.arange(m.npass) - m.pass0[m.sub]) * m.spb)
    assert np.array_equal(m.nloc, np.minimum(m.spb, nsf[m.sub] - m.sf0))
    # the search: passes, records and frames find their sub-channel, never one with an empty range
    assert np.array_equal(find(m.pass0, np.arange(m.npass)), m.sub)
    k = find(ri, np.arange(nrec))
    assert (r[k] > 0).all() and (np.arange(nrec) - ri[k] < nsf[k]).all() and np.array_equal(np.unique(k), np.flatnonzero(r > 0))
    nf = np.array([row[2] for row in rows], np.int64)
    frame0 = np.concatenate(([0], np.cumsum(nf)))[:-1]
    assert np.array_equal(find(frame0, np.arange(nf.sum())), np.repeat(np.arange(len(rows)), nf))
    return m


# ---- what a table makes the workgroups do ------------------------------------------------------------------------------

def trip_facts(m):
    """from the mirror: counts over the workgroups' trips and their hand-overs (trip t -> trip t + 1 of one workgroup)"""
    ntrips = np.array([len(t) for t in m.trips])
    hand = [(a, b) for t in m.trips for a, b in zip(t, t[1:])]
    a, b = (np.array(x, np.int64) for x in zip(*hand)) if hand else (np.zeros(0, np.int64),) * 2
    change = m.rsdims[a] != m.rsdims[b]
    last = np.flatnonzero(np.concatenate((m.sub[1:] != m.sub[:-1], [True]))) if m.npass else np.zeros(0, np.int64)
    return dict(
        npass=m.npass, grid=m.grid, min_trips=int(ntrips.min()), three_trips=int((ntrips >= 3).sum()),
        handovers=len(hand), width_changes=int(change.sum()),
        narrow_to_wide=int((m.rsdims[a] < m.rsdims[b]).sum()), wide_to_narrow=int((m.rsdims[a] > m.rsdims[b]).sum()),
        two_boundaries=sum(1 for t in m.trips if len(t) >= 3 and m.rsdims[t[0]] != m.rsdims[t[1]] != m.rsdims[t[2]]),
        partial_last_on_later_trip=int(((m.nloc[last] < m.spb[last]) & (m.trip_of[last] >= 1)).sum()))


def assert_trip_preconditions(f):
    """what tests/test_gpu_ens_trips.py needs of its table before its comparison means anything"""
    assert f["npass"] > 2 * f["grid"], f                      # the priority rotation is on
    assert f["min_trips"] >= 2, f
    assert 4 * f["three_trips"] >= f["grid"], f
    assert 4 * f["width_changes"] >= f["handovers"] > 0, f
    assert f["narrow_to_wide"] > 0 and f["wide_to_narrow"] > 0, f
    assert f["two_boundaries"] > 0, f
    assert f["partial_last_on_later_trip"] > 0, f


# ---- the table of the trips test, from the CU count -----------------------------------------------------------------------

TRIP_WIDTHS = (48, 3, 24, 7, 8, 1, 12, 3, 48, 7)  # a pass and the workgroup's next lie 4 to 5 entries apart
LONE_AT, LONE_WIDTH = 5, 2                        # one superframe of its own, uncorrectable, between entries 4 and 5
# distinct superframes per sub-channel, tiled: coprime to 256 // RSDims, so that a superframe meets every slot of a pass
PERIOD = {48: 7, 24: 7, 12: 11, 8: 13, 7: 13, 3: 31, 2: 1, 1: 97}
MIX = ("clean", "single", "real_1", "real_2", "real_3", "real_4", "real_5", "clean", "clean", "real_2", "single")


def trips_rows(cus):
    """(RSDims, superframes) per entry: 2 grid + grid / 4 and a few more passes in all, spread evenly over ten entries of
    interleaved widths whose last pass is half full, and in the middle an entry of one superframe"""
    grid = 4 * cus
    total = 2 * grid + grid // 4 + max(2, grid // 16)
    base, rem = divmod(total - 1, len(TRIP_WIDTHS))
    dims = []
    for k, r in enumerate(TRIP_WIDTHS):
        spb = RS_THREADS // r
        dims.append((r, (base + (k < rem)) * spb - spb // 2))
    dims.insert(LONE_AT, (LONE_WIDTH, 1))
    return dims


def period_blocks(pool, dims, lone=None):
    """per (RSDims, superframes) entry the block (P, 120 * RSDims) of its distinct superframes: superframe s of the entry
    is number s mod P.  Columns from rsdirect's pool: clean, 1 ... 5 errors and, in every fifth superframe, one column of
    an uncorrectable class.  The first and the last superframe of every entry are clean throughout - the neighbours of
    the entry `lone`, whose single superframe fails in its first column."""
    blocks = []
    for k, (r, nsf) in enumerate(dims):
        P = min(PERIOD[r], nsf)
        assert math.gcd(PERIOD[r], RS_THREADS // r) == 1
        idx = np.zeros((P, r), np.int64)
        for i in range(P):
            for j in range(r):
                if k == lone:
                    label = D.FAIL_CLASSES[0] if j == 0 else "clean"
                elif i in (0, (nsf - 1) % P):
                    label = "clean"
                elif i % 5 == 2 and j == (7 * i + k) % r:
                    label = D.FAIL_CLASSES[(i + k) % 3]
                else:
                    label = MIX[(3 * i + j + k + 1) % len(MIX)]
                idx[i, j] = pool.take(label)
        blocks.append(D.superframes(pool, idx))
    return blocks


def decode_periods(O, dims, blocks):
    """the oracle on the distinct superframes only -> per entry (ret (P,), out (P, 110 * RSDims), untouched bytes at the sentinel)"""
    return [O.rs_check_batch(b, r, np.full((b.shape[0], 110 * r), reffix.RS_SENTINEL, np.uint8)) for (r, _), b in zip(dims, blocks)]


def tiled_returns(dims, decoded):
    return np.concatenate([ret[np.arange(nsf) % ret.size] for (_, nsf), (ret, _) in zip(dims, decoded)]).astype(np.int32)


def assert_failures_on_every_trip(m, ret, lone_rec=None):
    """ret: the expected return value of every record.  Failures in passes that are a first, a second and a third trip;
    a pass whose workgroup held a failure in the same slot one trip earlier and now holds a superframe without one (what
    a value left in s_minfail would spoil), and the same for a corrected superframe (s_sum); the lone failing
    superframe is a later trip reached from another width, between clean superframes of its neighbours."""
    fail_trip, stale_fail, stale_sum = set(), 0, 0
    slot = lambda g: ret[m.rec[g]:m.rec[g] + m.nloc[g]]  # noqa: E731
    for g in range(m.npass):
        if (slot(g) < 0).any():
            fail_trip.add(int(m.trip_of[g]))
    for t in m.trips:
        for a, b in zip(t, t[1:]):
            n = min(m.nloc[a], m.nloc[b])
            stale_fail += int(((slot(a)[:n] < 0) & (slot(b)[:n] >= 0)).sum())
            stale_sum += int(((slot(a)[:n] > 0) & (slot(b)[:n] == 0)).sum())
    assert {0, 1, 2} <= fail_trip and stale_fail >= 8 and stale_sum >= 8, (fail_trip, stale_fail, stale_sum)
    if lone_rec is not None:
        g = int(np.flatnonzero(m.rec == lone_rec)[0])
        assert m.nloc[g] == 1 and m.trip_of[g] >= 1 and m.rsdims[g - m.grid] != m.rsdims[g]
        assert ret[lone_rec - 1:lone_rec + 2].tolist() == [0, -1, 0]
        assert m.sub[g - 1] == m.sub[g] - 1 and m.sub[g + 1] == m.sub[g] + 1  # the neighbours' passes: other sub-channels
        assert m.trip_of[g - 1] >= 1 and m.trip_of[g + 1] >= 1
        assert m.rsdims[g - 1 - m.grid] != m.rsdims[g - 1] and m.rsdims[g + 1 - m.grid] != m.rsdims[g + 1]


# ---- the uniform kernel's later trips (rs_kernel): one entry, the same geometry ----------------------------------------

UNIFORM_CASES = [(12, 0), (7, 0), (8, 1)]  # (RSDims, byte offset of p and out): dword copy-out; byte path; copy_linear in, bytes out


def uniform_dims(r, cus):
    grid, spb = 4 * cus, RS_THREADS // r
    return [(r, (grid + grid // 4 + 3) * spb - spb // 2)]


# ---- table shapes ---------------------------------------------------------------------------------------------------------

def mixed_64():
    """64 entries: RSDims 1 ... 48 all present, one to three superframes each (RSDims 1 and 2: up to 7), every seventh
    entry not DAB+ - first and last among them, and 62, 63 in a row"""
    rows, c = [], 0
    for k in range(MAX_SUBCH):
        if k % 7 == 0 or k == 62:
            rows.append(plain(8 * (1 + (k * 5) % 24), 1 + k % 3))
        else:
            r = 1 + (c * 29) % 48  # 29 and 48 are coprime: the 53 DAB+ entries hold every width
            rows.append(dab(r, 1 + (k % 3) + (4 if r <= 2 else 0)))
            c += 1
    return rows


EDGE_TABLES = {
    "mixed_64": mixed_64(),
    "plain_first": [plain(8, 1), dab(3, 2), dab(8, 33)],
    "plain_last": [dab(8, 33), dab(3, 2), plain(1536, 3)],
    "plain_adjacent": [dab(1, 5), plain(192, 2), plain(8, 1), dab(7, 2), plain(64, 1), plain(72, 5), dab(24, 1)],
    "rsdims_1_full": [dab(1, 256), plain(8, 1), dab(1, 257)],   # a pass exactly full, every s_minfail slot live; and one more
    "rsdims_2_full": [dab(2, 128), dab(2, 129)],
    "rsdims_48_full": [dab(48, 5), plain(24, 2), dab(48, 6)],
}
ONLY_PLAIN = [plain(8, 1), plain(1536, 3), plain(192, 7)]


def edge_rs_blocks(pool, rows):
    """per entry its RS input block from rsdirect's columns (not DAB+: None): a failing column in every fourth superframe,
    and in the first and last superframe of an entry of more than 8 (slots 0 and 255 of a full RSDims 1 pass)"""
    blocks = []
    for k, (_, r, nframes) in enumerate(rows):
        if not r:
            blocks.append(None)
            continue
        nsf = nframes // 5
        idx = np.zeros((nsf, r), np.int64)
        for s in range(nsf):
            fails = s % 4 == 1 or (nsf > 8 and s in (0, nsf - 1))
            for j in range(r):
                label = D.FAIL_CLASSES[(s + k) % 3] if fails and j == (5 * s + k) % r else MIX[(3 * s + j + k + 1) % len(MIX)]
                idx[s, j] = pool.take(label)
        blocks.append(D.superframes(pool, idx))
    return blocks


# ---- tests ----------------------------------------------------------------------------------------------------------------

CUS = (1, 8, 256, 304)


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("name", sorted(EDGE_TABLES) + ["only_plain"])
def test_mirror_on_the_edge_tables(V, name, cus):
    rows = ONLY_PLAIN if name == "only_plain" else EDGE_TABLES[name]
    m = check_mirror(V, rows, cus)
    if name == "only_plain":
        assert m.npass == 0 and m.grid == 0 and int(V.ensemble_layout(table(V, rows))["nrec"]) == 0
    if name == "mixed_64":
        assert len(rows) == MAX_SUBCH and {row[1] for row in rows} == set(range(49))
        assert not rows[0][1] and not rows[63][1] and not rows[62][1]
    if name.endswith("_full"):
        r = rows[0][1]
        assert m.nloc.tolist() == [256 // r, 256 // r, 1]  # exactly full; full and one superframe over


@pytest.mark.parametrize("cus", CUS)
def test_mirror_on_the_trips_table(V, cus):
    dims = trips_rows(cus)
    m = check_mirror(V, [dab(r, n) for r, n in dims], cus)
    assert 7 <= len(dims) <= 12 and max(np.bincount(m.sub)) <= 400
    lay = V.ensemble_layout(table(V, [dab(r, n) for r, n in dims]))
    assert int(lay["work_bytes"]) + 2 * int(lay["rs_bytes"]) < 256 << 20  # input, output, and one more output's worth


@pytest.mark.parametrize("cus", [8, 256, 304])
def test_trips_table_meets_the_preconditions(V, O, cus):
    """the GPU test's table for this CU count reaches what it is for: later trips, width changes in both directions,
    failures on each trip and in the slots a stale s_minfail / s_sum would spoil"""
    dims = trips_rows(cus)
    rows = [dab(r, n) for r, n in dims]
    lay = V.ensemble_layout(table(V, rows))
    m = passes(rows, cus, lay)
    assert_trip_preconditions(trip_facts(m))
    blocks = period_blocks(D.Pool(), dims, lone=LONE_AT)
    ret = tiled_returns(dims, decode_periods(O, dims, blocks))
    assert ret.size == int(lay["nrec"])
    assert_failures_on_every_trip(m, ret, lone_rec=int(lay["rec_index"][LONE_AT]))
    assert max(ret) >= 5 * 3 and {1, 2, 3, 4, 5} <= set(ret.tolist())


@pytest.mark.parametrize("cus", [8, 256, 304])
@pytest.mark.parametrize("r,offset", UNIFORM_CASES)
def test_uniform_cases_reach_a_second_trip(V, O, r, offset, cus):
    dims = uniform_dims(r, cus)
    rows = [dab(*dims[0])]
    m = passes(rows, cus, V.ensemble_layout(table(V, rows)))
    f = trip_facts(m)
    assert f["grid"] == 4 * cus < f["npass"] and f["min_trips"] >= 1 and 4 * sum(len(t) >= 2 for t in m.trips) >= f["grid"]
    assert m.nloc[-1] < m.spb[-1] and m.trip_of[-1] == 1
    ret = tiled_returns(dims, decode_periods(O, dims, period_blocks(D.Pool(), dims)))
    fail_trip = {int(m.trip_of[g]) for g in range(m.npass) if (ret[m.rec[g]:m.rec[g] + m.nloc[g]] < 0).any()}
    assert fail_trip == {0, 1}
    out_sz = 110 * r
    assert {12: out_sz % 16 == 8, 7: out_sz % 4 != 0, 8: out_sz % 16 == 0}[r]


def test_the_existing_table_never_makes_a_second_trip(V):
    """the gap this file is about: the table of tests/test_gpu_ensemble.py has 8 passes, one per workgroup"""
    rows = [dab(r, n) for r, n in [(1, 3), (3, 1), (7, 2), (8, 37), (24, 2), (48, 6)]]
    m = passes(rows, 256, V.ensemble_layout(table(V, rows)))
    assert m.npass == 8 == m.grid and all(len(t) == 1 for t in m.trips)
