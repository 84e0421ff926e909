"""CPU-only: the syndrome-directed RS(120,110) columns of tests/rsdirect.py - the generator's own checks, every class
through the oracle's DECODE_RS and (where oracle/_ref exists) the reference's, and the conditions under which the classes
test what they are meant to.  The GPU side is tests/test_gpu_rs_paths.py.

What a class must return where construction fixes it:
  real_d, pad_d_m   d, and the decoded column is the input with Y_j XORed at the roots outside the padding (numpy alone)
  deg2_noroot, deg2_double, nosplit_d   -1 (the locator has fewer roots than its degree)
  deg2_r0           2 (a root at X = 1: closed-form index 0 is the scan's index 255)
  short_2, short_3  1 (the LFSR is longer than the locator's degree; only deg_lambda == count is checked)
  num1_zero_d       d, and the byte of the first root stays as it came (Forney's `num1 == 0` patches nothing)
  deg6_ok           6: THE REFERENCE ACCEPTS LOCATORS ABOVE DEGREE 5 when they split
Everything else is whatever the reference does; the oracle and the committed digests decide.
"""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import _vitpkg  # noqa: E402
import reffix  # noqa: E402
import rsdirect as D  # noqa: E402

EXPECTED_LABELS = (["real_%d" % d for d in range(1, 6)] + ["pad_%d_%d" % (d, m) for d in range(1, 6) for m in range(1, d + 1)]
                   + ["deg2_noroot", "deg2_double", "deg2_r0", "nosplit_3", "nosplit_4", "nosplit_5"]
                   + ["short_%d" % k for k in range(2, 10)] + ["zero_s0", "zero_s1", "num1_zero_1", "num1_zero_2", "num1_zero_3", "deg6_ok", "deg6_bad", "deg7", "deg8", "deg9", "deg10"]
                   + ["over_%d" % w for w in range(6, 11)] + ["random"])


@pytest.fixture(scope="module")
def R():
    mod = _vitpkg.load_ref()
    if mod.reference_dir() is None and not mod.available():
        pytest.skip("no oracle/_ref and no reference checkout to build it from ($VIT_REFERENCE_DIR or ../reference)")
    assert mod.build(), "oracle/_ref could not be built"
    return mod


@pytest.fixture(scope="module")
def oracle_results(O):
    """label -> (ret, patched columns) from the oracle's DECODE_RS, every column of every class"""
    return {label: D.decode_columns(O.rs_decode_word, k.words) for label, k in D.classes().items()}


def test_generator_self_checks():
    C = D.classes()
    assert list(C) == EXPECTED_LABELS
    assert set(D.VALUE_CLASSES) == {label for label, k in C.items() if k.expect is not None}
    # the Vandermonde inverses really are inverses, for every position set
    for pos in D.POSITION_SETS:
        vinv = D.vandermonde_inverse(pos)
        V = np.array([[reffix.ALPHA[(i * (119 - p)) % 255] for p in pos] for i in range(10)])
        prod = np.bitwise_xor.reduce(D.gmul(V[:, :, None], vinv[None, :, :]), axis=1)
        assert np.array_equal(prod, np.eye(10, dtype=np.uint8)), pos
    # the columns have the syndromes they were built for (the reference's Horner sums, recomputed), on all three position sets
    for label, k in C.items():
        if k.syn is not None:
            assert np.array_equal(D.horner_syndromes(k.words), k.syn), label
    assert not D.horner_syndromes(D.fillers()["clean"].words).any()
    # class constraints
    for label, k in C.items():
        if label.startswith(("real_", "pad_")):
            d, m = (int(label[5:]), 0) if label.startswith("real_") else (int(label[4]), int(label[6]))
            assert k.roots.shape == (len(k), d) and ((k.roots <= D.PAD).sum(axis=1) == m).all(), label
            assert all(len(set(r)) == d for r in k.roots.tolist()) and k.roots.min() >= 1 and k.roots.max() <= 255, label
            for i, fixed in enumerate(D._FIXED_ROOTS.get(label, [])):
                assert tuple(k.roots[i]) == fixed
    for z, label in ((5, "deg6_bad"), (6, "deg7"), (7, "deg8"), (8, "deg9"), (9, "deg10")):
        assert not C[label].syn[:, :z].any() and C[label].syn[:, z].all()
    for k in range(2, 10):  # geometric except for S_k
        s = C["short_%d" % k].syn.astype(np.int64)
        step = D.gmul(s[:, :-1], D.gmul(s[:, 1], D.ginv(s[:, 0]))[:, None]) == s[:, 1:]  # S_i X == S_(i+1), X = S_1 / S_0
        off = [i for i in range(9) if i + 1 == k or i == k]
        assert step[:, [i for i in range(9) if i not in off]].all() and not step[:, off].any(), k
    assert not C["zero_s0"].syn[:, 0].any() and not C["zero_s1"].syn[:, 1].any()
    groups = {label: [len({(r - 1) // 4 for r in row}) for row in C[label].roots[:4].tolist()] for label in ("real_2", "real_3", "real_4")}
    assert 1 in groups["real_2"] and 1 in groups["real_3"] and 1 in groups["real_4"]  # 2, 3, 4 roots in one group 4L+1..4L+4


def test_generator_is_deterministic():
    """the columns are the committed ones: class by class against the digests in reference_provenance.json, and the
    pinned tables' inputs against the input digests in reference_rs_paths.npy"""
    with open(reffix.PROVENANCE_JSON) as f:
        prov = json.load(f)["rs_paths"]
    assert D.class_digests() == prov["class_digests"]
    rows = np.load(D.RS_PATHS_NPY)
    tabs = D.pinned_tables()
    assert rows.shape == (sum(t.nsf for t in tabs), len(reffix.RS_COLS)) and rows.dtype == np.uint64
    assert rows.shape[0] == prov["superframes"]
    assert os.path.getsize(D.RS_PATHS_NPY) < os.path.getsize(os.path.join(reffix.GOLD, "golden.json"))
    at = 0
    for t in tabs:
        assert (rows[at:at + t.nsf, 0] == t.rsdims).all(), t.name
        assert np.array_equal(reffix.fnv1a64_rows(list(t.p)), rows[at:at + t.nsf, 3]), "input generator drifted: " + t.name
        at += t.nsf


def test_every_class_through_the_oracle(oracle_results):
    """the "expected" column of the class table, the numpy-only decoded columns, and non-vacuity"""
    C = D.classes()
    for label, k in C.items():
        ret, fix = oracle_results[label]
        if k.expect is not None:
            assert (ret == k.expect).all(), (label, np.flatnonzero(ret != k.expect)[:8])
        if k.want is not None:
            assert np.array_equal(fix, k.want), label  # all 120 bytes: parity rows are patched too
        assert np.array_equal(fix[ret < 0], k.words[ret < 0]), label  # a failed column is left as it came
    for d in (1, 2, 3):  # `num1 == 0`: the first root's byte is left alone, at most d - 1 bytes change
        k, (ret, fix) = C["num1_zero_%d" % d], oracle_results["num1_zero_%d" % d]
        first = k.roots[:, 0] - D.PAD - 1
        rows = np.arange(len(k))
        assert (fix[rows, first] == k.words[rows, first]).all() and ((fix != k.words).sum(axis=1) <= d - 1).all(), d
    counts = D.non_vacuity({label: r[0] for label, r in oracle_results.items()})
    # Forney's quirks, counted (no floor): accepted columns that patch fewer bytes than they have roots outside the padding
    num1_zero = 0
    for label, k in C.items():
        if k.roots is not None:
            ret, fix = oracle_results[label]
            num1_zero += int(((ret >= 0) & ((fix != k.words).sum(axis=1) < (k.roots > D.PAD).sum(axis=1))).sum())
    print("RS paths:", counts, "num1 == 0 on a chosen root:", num1_zero)
    with open(reffix.PROVENANCE_JSON) as f:
        assert counts == json.load(f)["rs_paths"]["reference_counts"]  # the oracle counts what the reference build counted


def test_every_class_oracle_equals_reference_build(R, oracle_results):
    """every column: return value and all 120 bytes, oracle == the reference's DECODE_RS"""
    total = 0
    for label, k in D.classes().items():
        ret, fix = R.rs_decode_words(k.words)
        ret_o, fix_o = oracle_results[label]
        assert np.array_equal(ret, ret_o), (label, np.flatnonzero(ret != ret_o)[:8])
        assert np.array_equal(fix, fix_o), (label, np.flatnonzero((fix != fix_o).any(axis=1))[:8])
        total += len(k)
    D.non_vacuity({label: R.rs_decode_words(k.words)[0] for label, k in D.classes().items()})
    assert total >= 30000


def test_tables_oracle_equals_reference_build(R, O):
    """the superframe tables of the GPU test (the wave-company table by a stride: it repeats the classes' columns)"""
    pool = D.Pool()
    tabs = D.pinned_tables() + [D.per_column_table(pool)]
    comp = D.company_table(pool)
    for t in tabs:
        init = np.full((t.nsf, 110 * t.rsdims), reffix.RS_SENTINEL, np.uint8)
        ret, out = R.rs_check_batch(t.p, t.rsdims, init)
        ret_o, out_o = O.rs_check_batch(t.p, t.rsdims, init)
        assert np.array_equal(ret, ret_o) and np.array_equal(out, out_o), t.name
    sub = comp.p[::5]
    init = np.full((sub.shape[0], 110), reffix.RS_SENTINEL, np.uint8)
    ret, out = R.rs_check_batch(sub, 1, init)
    ret_o, out_o = O.rs_check_batch(sub, 1, init)
    assert np.array_equal(ret, ret_o) and np.array_equal(out, out_o)


def test_table_contexts_are_reached(O, oracle_results):
    """the coverage the GPU test relies on, from the oracle's classification of the tables' own columns"""
    pool = D.Pool()
    cells = D.table_cells(pool, [D.company_table(pool)] + [D.first_failure_table(r, pool) for r in D.FIRST_FAILURE_DIMS]
                          + [D.wide_table(r, pool) for r in D.WIDE_DIMS] + [D.export_table(r, pool) for r in D.EXPORT_DIMS],
                          D.pool_returns(pool, {label: r[0] for label, r in oracle_results.items()}))
    D.assert_cells(cells)
