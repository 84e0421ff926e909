"""CPU: the syndrome-directed RS(204,188) rows of tests/fecdirect.py - every row takes the path its label names (by the
classifier), the model decodes it as construction says, the kernel's "cut at degree 8" Berlekamp-Massey fails exactly
where the full-length one says L > 8 or deg != L, the host twin vit_packet_fec_frame_host equals the model on the whole
set, and the vectorised sync model equals the looped one."""
import collections

import numpy as np

import fecdirect as fd
from test_packet_host import (FEC_FRAME_BYTES, FEC_SLOTS, NCODE, ROWS, SLOT, TCORR, decode_row_model, fec_frame_model, same,
                              sync_model, syndromes)


def test_directed_rows_take_their_paths():
    D = fd.directed_set()
    have = collections.Counter(e.name for e in D)
    want = fd.expected_counts()
    for name, n in want.items():
        assert have[name] == n, (name, have[name], n)
    zd = [e for e in D if e.group == "zero_dsc"]
    assert len(zd) >= 8 and sum("jump>=2" in e.need for e in zd) >= 1
    assert set(have) - set(want) == {e.name for e in zd}
    assert len({e.row.tobytes() for e in D}) == len(D)
    labels = collections.Counter()
    for e in D:
        got = fd.classify(e.row)
        assert e.need <= got, (e.name, sorted(e.need - got), sorted(got))
        labels.update(got)
    # the cells of the list, counted from the classifier's labels alone
    assert labels["S0=0"] >= 7 + 14 and all(labels["lead%d" % m] >= 2 for m in range(1, 8))
    assert all(labels["lone_S%d=0" % k] >= 1 for k in range(1, 16))
    assert labels["zero_dsc_mid"] >= 8 and labels["jump>=2"] >= 1
    assert all(labels["lam1=0@L%d" % L] >= 1 for L in range(3, 9)) and all(labels["lam%d=0@L8" % j] >= 1 for j in range(1, 8))
    assert all(labels["L%d" % L] >= 1 for L in range(1, 17)) and labels["L>8"] >= 8 + 8
    assert all(labels["root@%d" % d] >= 1 for d in range(NCODE)), "every real position is a root of some row"
    assert labels["root@204"] >= 1 and labels["root@254"] >= 2 and labels["repeated_root"] >= 3 and labels["few_roots"] >= 6
    for L in (1, 2, 4, 8):
        assert any({"deg<L", "L%d" % L} <= fd.classify(e.row) for e in D if e.group == "deg<L"), L
    assert labels["pad_roots1"] >= 2 + 1 + 2 + 3 and labels["pad_roots8"] >= 1
    # the late jumps go from n to k + 1 - n in one step
    for e in D:
        if e.group == "late_jump":
            n, k = int(e.name.split("_")[2][1:]), int(e.name.split("_")[3][1:])
            L, deg, lam, steps = fd.bm_trace(syndromes(e.row))
            assert L == k + 1 - n > TCORR and steps[k] == (True, True, k + 1 - 2 * n)
    # the seam rows: eight roots, the named one among them
    for e in D:
        if e.group == "seam":
            got = fd.classify(e.row)
            assert "roots8" in got and (set("root@%d" % d for d in fd.SEAMS) <= got if e.name == "seam_all" else True)


def test_model_decodes_the_directed_rows_as_constructed():
    seen = collections.Counter()
    for e in fd.directed_set():
        got, ne = decode_row_model(e.row)
        assert ne == e.nerr, (e.name, ne, e.nerr)
        assert np.array_equal(got, e.want), e.name
        if ne > 0:
            assert not syndromes(got).any() and int((got != e.row).sum()) == ne
        seen[(e.group, ne)] += 1
    for g in ("L>8", "late_jump", "deg<L", "irreducible", "repeated", "pad_k1", "pad_all", "pad_254", "padding_root"):
        assert {n for (grp, n) in seen if grp == g} == {-1}, g
    assert {n for (grp, n) in seen if grp == "pad_204"} == {3, -1}
    assert {n for (grp, n) in seen if grp == "s0_zero"} == set(range(2, 9))
    # single errors: every position, every value
    singles = [e for e in fd.directed_set() if e.group == "single"]
    diffs = [(int(np.flatnonzero(e.row != e.want)[0]), int((e.row ^ e.want).max())) for e in singles]
    assert {NCODE - 1 - k for k, _ in diffs} == set(range(NCODE)) and {v for _, v in diffs} == set(range(1, 256))


def test_cut_at_degree_8_fails_exactly_where_the_full_trace_says():
    """vit_fec_kernel keeps nine coefficients of Lambda and B.  Its claim: a term above x^8 means L > 8, which fails anyway.
    So the cut recursion must be `bad` exactly when the full one has L > 8 or deg != L, and otherwise agree on Lambda."""
    rng = np.random.default_rng(8)
    rows = [e.row for e in fd.directed_set()]
    rows += list(fd.heavy_rows(rng, 3000))
    light = fd.clean_rows(rng, 1000)
    for k in range(1000):
        w = 1 + k % 8
        light[k, rng.permutation(NCODE)[:w]] ^= rng.integers(1, 256, w, dtype=np.uint8)
    rows += list(light)
    S = syndromes(np.stack(rows))
    S = np.concatenate([S, rng.integers(0, 256, (1000, 16), dtype=np.uint8)])  # (any vector is some row's)
    S = S.tolist()
    for k in range(1500):  # L > 8 in bulk: leading zeros, and few errors' power sums with one later word altered
        m = 6 + k % 10
        S.append([0] * m + [int(x) for x in rng.integers(0, 256, 16 - m)])
        n = 1 + k % 7
        s = fd.power_sums(fd.random_degs(rng, n, hi=255), [int(x) for x in rng.integers(1, 256, n)])
        s[int(rng.integers(2 * n, 16))] ^= int(rng.integers(1, 256))
        S.append(s)
    nbad = ngood = nover = 0
    for s in S:
        if not any(s):
            continue
        L, deg, lam, steps = fd.bm_trace(s)
        Lc, degc, lamc, badc = fd.bm_trace_cut(s)
        bad = L > TCORR or deg != L
        assert badc == bad, (s, L, deg, Lc, degc)
        if not badc:
            assert (Lc, degc) == (L, deg) and lamc == lam[:TCORR + 1] and not any(lam[TCORR + 1:]), s
            ngood += 1
        else:
            nbad += 1
            nover += L > TCORR
    # (sixteen generic words have linear complexity 8: the heavy rows mostly end at L = deg = 8 and fail by their roots;
    # the directed set brings the 16 rows with L > 8 and the 8 with deg < L)
    assert ngood >= 4000 and nover >= 1000 and nbad - nover >= 8, (ngood, nover, nbad)


def test_row_model_cache_is_the_frame_model():
    rng = np.random.default_rng(11)
    D = fd.directed_set()
    rows = fd.clean_rows(rng, 3 * ROWS).reshape(3, ROWS, NCODE)
    for k, e in enumerate(D[::17][:24]):
        rows[k % 3, (5 * k) % ROWS] = e.row
    frames = fd.frames_of_rows(rows)
    frames[1, fd.FEC_DATA_BYTES + SLOT * 4] ^= 0x80
    frames[2, -3:] = 7
    got, rec = fd.RowModel().frames(frames)
    for f in range(3):
        want, wrec = fec_frame_model(frames[f])
        assert np.array_equal(got[f], want) and rec[f].tobytes() == wrec.tobytes()
    assert rec["hdr_ok"].tolist() == [0x1FF, 0x1FF ^ 16, 0x1FF]


def test_host_twin_on_the_directed_set(V):
    rng = np.random.default_rng(12)
    D = fd.directed_set()
    n = -(-len(D) // ROWS)
    rows = fd.clean_rows(rng, n * ROWS)
    for k, e in enumerate(D):
        rows[k] = e.row
    frames = fd.frames_of_rows(rows.reshape(n, ROWS, NCODE))
    model = fd.RowModel()
    nerr = []
    for f in range(n):
        want, wrec = fec_frame_model(frames[f]) if f % 8 == 0 else [x[0] for x in model.frames(frames[f])]
        got, grec = V.packet_fec_frame_host(frames[f])
        assert np.array_equal(got, want), (f, np.flatnonzero(got != want)[:8])
        assert grec.tobytes() == wrec.tobytes(), (f, grec, wrec)
        nerr += wrec["nerr"].tolist()
    assert nerr[:len(D)] == [e.nerr for e in D]
    # rows beyond the code's reach, the bulk the GPU test compares through the host twin
    heavy = fd.frames_of_rows(fd.heavy_rows(rng, 20 * ROWS).reshape(20, ROWS, NCODE))
    want, wrec = model.frames(heavy)
    for f in range(20):
        got, grec = V.packet_fec_frame_host(heavy[f])
        assert np.array_equal(got, want[f]) and grec.tobytes() == wrec[f].tobytes()


def test_sync_model_fast_is_sync_model():
    for nslots in (1, 9, 103, 104, 1000):
        rng = np.random.default_rng(nslots)
        for phase in (0, 50, 102):
            st = fd.sync_stream(rng, nslots, phase)
            assert same(fd.sync_model_fast(st), sync_model(st)), (nslots, phase)
        st = rng.integers(0, 256, SLOT * nslots + 5, dtype=np.uint8)
        assert same(fd.sync_model_fast(st), sync_model(st))
    assert FEC_FRAME_BYTES == SLOT * FEC_SLOTS
