"""GPU: every path of the RS(120,110) correction tree (csrc/rs_kernels.hip: rs_correct, chien_wave, chien_quad,
chien_log, Forney) with the syndrome-directed columns of tests/rsdirect.py - columns that choose their locator (degree,
root set, roots in the virtual padding, repeated or missing roots, degree 6 and above that the reference ACCEPTS) and the
wave they sit in, instead of waiting for "codeword plus random errors" to produce them.

Everything goes through the C ABI.  Outputs start as a sentinel with 64 guard bytes on both sides, d_ret as a marker;
every return value and every output byte is compared with the oracle, the seeded tables also with the committed results
of the reference's own rschecksf.cpp (tests/golden/reference_rs_paths.npy) without any oracle.  Launches are few and
large: one table per RSDims and context.
"""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  before libviterbi.so is loaded: a run of this module alone must bring up torch's HIP runtime first

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import reffix  # noqa: E402
import rsdirect as D  # noqa: E402

GUARD = 64
MARKER = 12345


@pytest.fixture
def pool():
    """a fresh one per test: a table does not depend on which tests ran before"""
    return D.Pool()


@pytest.fixture(scope="module")
def oracle_ret(O):
    """label -> the oracle's return value for every column of the class; non-vacuity asserted on it"""
    ret_of = {label: D.decode_columns(O.rs_decode_word, k.words)[0] for label, k in D.classes().items()}
    print("RS paths:", D.non_vacuity(ret_of))
    return ret_of


def _dev(V, torch, p, rsdims):
    """vit_rs_batch_dev on sentinel-filled, guarded output -> (ret, out (nsf, 110 * rsdims))"""
    nsf = p.shape[0]
    n = nsf * 110 * rsdims
    d_o = torch.full((n + 2 * GUARD,), reffix.RS_SENTINEL, dtype=torch.uint8, device="cuda")
    d_ret = torch.full((nsf + 2,), MARKER, dtype=torch.int32, device="cuda")
    V.rs_batch_dev(torch.from_numpy(p).cuda(), d_o[GUARD:], d_ret[1:], rsdims, nsf)
    torch.cuda.synchronize()
    got, ret = d_o.cpu().numpy(), d_ret.cpu().numpy()
    assert (got[:GUARD] == reffix.RS_SENTINEL).all() and (got[GUARD + n:] == reffix.RS_SENTINEL).all(), "wrote outside the output"
    assert ret[0] == MARKER and ret[-1] == MARKER, "wrote outside d_ret"
    return ret[1:-1].copy(), got[GUARD:GUARD + n].reshape(nsf, 110 * rsdims)


def _where(t, pool, bad):
    """the first differing superframes: (superframe, classes of its columns)"""
    names = []
    for s in bad[:6]:
        labs = [pool.labels[i] for i in pool.label_of[t.idx[s]]]
        special = [(j, l) for j, l in enumerate(labs) if l not in ("clean", "single")][:6]
        names.append((int(s), special))
    return names


def _compare(t, pool, ret, out, want_ret, want_out, what):
    bad = np.flatnonzero(ret != want_ret)
    assert bad.size == 0, "%s %s: %d return values differ, (superframe, [(column, class)]): %s; got %s want %s" % (
        what, t.name, bad.size, _where(t, pool, bad), ret[bad[:6]], want_ret[bad[:6]])
    bad = np.flatnonzero((out != want_out).any(axis=1))
    assert bad.size == 0, "%s %s: %d outputs differ, (superframe, [(column, class)]): %s" % (what, t.name, bad.size, _where(t, pool, bad))


def _oracle(O, t):
    return O.rs_check_batch(t.p, t.rsdims, np.full((t.nsf, 110 * t.rsdims), reffix.RS_SENTINEL, np.uint8))


def test_per_column(V, O, torch_cuda, pool, oracle_ret):
    """RSDims 1: every column of every class a superframe of its own (256 per pass, a wave = 64 consecutive ones, no
    first-failure rule in the way), the `random` volume included, one launch.  Besides the oracle: where construction
    fixes the result (rsdirect.VALUE_CLASSES; real_d / pad_d_m to the byte) it is checked from numpy alone."""
    t = D.per_column_table(pool)
    ret, out = _dev(V, torch_cuda, t.p, 1)
    at = 0
    for label, k in D.classes().items():
        r, o = ret[at:at + len(k)], out[at:at + len(k)]
        if k.expect is not None:
            assert (r == k.expect).all(), (label, np.flatnonzero(r != k.expect)[:8], r[r != k.expect][:8])
        if k.want is not None:
            assert np.array_equal(o, k.want[:, :110]), (label, np.flatnonzero((o != k.want[:, :110]).any(axis=1))[:8])
        assert np.array_equal(r, oracle_ret[label]), (label, np.flatnonzero(r != oracle_ret[label])[:8])
        at += len(k)
    assert at == t.nsf
    want_ret, want_out = _oracle(O, t)
    _compare(t, pool, ret, out, want_ret, want_out, "dev")
    cells = D.table_cells(pool, [t], D.pool_returns(pool, oracle_ret))
    for label in D.classes():
        assert cells[("per_column", "column", label)] >= 64


def test_wave_company(V, O, torch_cuda, pool, oracle_ret):
    """one special column (each class in turn) at lane 0, 31 and 63 of a wave whose other 63 columns are clean, single
    errors, h columns of degree 3 resp. 4..5 on both sides of the switch between chien_wave and chien_quad, the same
    with a degree-6 locator in the wave (chien_log for every heavy lane), or 63 accepted degree-6 columns"""
    t = D.company_table(pool)
    ret, out = _dev(V, torch_cuda, t.p, 1)
    want_ret, want_out = _oracle(O, t)
    bad = np.flatnonzero((ret != want_ret) | (out != want_out).any(axis=1))
    if bad.size:
        ctx = D.company_contexts()
        per = 3 * len(D.classes()) * 64
        rows = [(ctx[b // per][0], list(D.classes())[(b % per) // 192], "lane %d" % (b % 64), pool.labels[pool.label_of[t.idx[b, 0]]],
                 int(ret[b]), int(want_ret[b])) for b in bad[:12]]
        pytest.fail("%d columns differ; (context, special class of the wave, lane, class of the column, got, want): %s" % (bad.size, rows))
    D.assert_cells(D.table_cells(pool, [t], D.pool_returns(pool, oracle_ret)))


@pytest.mark.parametrize("rsdims", D.FIRST_FAILURE_DIMS)
def test_first_failure_across_forms(V, O, torch_cuda, pool, oracle_ret, rsdims):
    """the first failing column is a closed-form one (enters chien_wave as `failed`), one that fails inside chien_wave, one
    that fails in chien_log; accepted special columns before it are written and summed, after it stay sentinel; failures
    in either wavefront of a superframe that straddles two; a partial last group.  Device and host entry."""
    t = D.first_failure_table(rsdims, pool)
    spb = max(1, 256 // rsdims)
    assert spb == 1 or t.nsf % spb, "the last group of the launch must be partial"
    want_ret, want_out = _oracle(O, t)
    ret, out = _dev(V, torch_cuda, t.p, rsdims)
    _compare(t, pool, ret, out, want_ret, want_out, "dev")
    ret, out = V.rs_batch_host(t.p, rsdims, out_init=np.full_like(want_out, reffix.RS_SENTINEL))
    _compare(t, pool, ret, out, want_ret, want_out, "host")
    # what the table is for, on the oracle's output: the failing column and everything behind it unwritten
    o3 = want_out.reshape(t.nsf, 110, rsdims)
    for ctx, label, sf, col in t.marks:
        if ctx == "first_failure":
            assert want_ret[sf] == -1 and (o3[sf, :, col:] == reffix.RS_SENTINEL).all(), (sf, col)
    D.assert_cells(D.table_cells(pool, [t], D.pool_returns(pool, oracle_ret)))


@pytest.mark.parametrize("rsdims", D.WIDE_DIMS)
def test_wide_kernel(V, O, torch_cuda, pool, oracle_ret, rsdims):
    """rs_kernel_wide: special columns in the first, a middle and the last 256-column chunk, a failure in the second chunk
    with accepted special columns before and after it, whole runs of one class across a chunk boundary"""
    t = D.wide_table(rsdims, pool)
    want_ret, want_out = _oracle(O, t)
    ret, out = _dev(V, torch_cuda, t.p, rsdims)
    _compare(t, pool, ret, out, want_ret, want_out, "dev")
    ret, out = V.rs_batch_host(t.p, rsdims, out_init=np.full_like(want_out, reffix.RS_SENTINEL))
    _compare(t, pool, ret, out, want_ret, want_out, "host")
    D.assert_cells(D.table_cells(pool, [t], D.pool_returns(pool, oracle_ret)))


@pytest.mark.parametrize("rsdims", D.EXPORT_DIMS)
def test_export(V, O, torch_cuda, pool, oracle_ret, rsdims):
    """RScheckSuperframe, one superframe per class: the polled single-workgroup form (RSDims <= 256) and the plain launch
    above it"""
    t = D.export_table(rsdims, pool)
    want_ret, want_out = _oracle(O, t)
    for s in range(t.nsf):
        buf = np.full(110 * rsdims + 2 * GUARD, reffix.RS_SENTINEL, np.uint8)
        rc, _ = V.RScheckSuperframe(t.p[s], 0, rsdims, buf[GUARD:])
        assert rc == int(want_ret[s]), (rsdims, s, _where(t, pool, [s]), rc, int(want_ret[s]))
        assert np.array_equal(buf[GUARD:-GUARD], want_out[s]), (rsdims, s, _where(t, pool, [s]))
        assert (buf[:GUARD] == reffix.RS_SENTINEL).all() and (buf[-GUARD:] == reffix.RS_SENTINEL).all()
    D.assert_cells(D.table_cells(pool, [t], D.pool_returns(pool, oracle_ret)))


def test_host_entry_per_column(V, O, torch_cuda, pool):
    """vit_rs_batch_host at RSDims 1: 64 columns of every class"""
    t = D.per_column_table(pool, limit=64)
    want_ret, want_out = _oracle(O, t)
    ret, out = V.rs_batch_host(t.p, 1, out_init=np.full_like(want_out, reffix.RS_SENTINEL))
    _compare(t, pool, ret, out, want_ret, want_out, "host")


def test_pinned_tables_against_the_reference_digests(V, torch_cuda):
    """no oracle: the committed return values and output digests of the reference's own rschecksf.cpp"""
    rows = np.load(D.RS_PATHS_NPY)
    tabs = D.pinned_tables()
    assert rows.shape == (sum(t.nsf for t in tabs), len(reffix.RS_COLS))
    at = 0
    for t in tabs:
        want = rows[at:at + t.nsf]
        at += t.nsf
        assert (want[:, 0] == t.rsdims).all()
        assert np.array_equal(reffix.fnv1a64_rows(list(t.p)), want[:, 3]), "RS input generator drifted: " + t.name
        ret, out = _dev(V, torch_cuda, t.p, t.rsdims)
        want_ret = np.ascontiguousarray(want[:, 1]).view(np.int64)
        bad = np.flatnonzero(ret.astype(np.int64) != want_ret)
        assert bad.size == 0, (t.name, bad[:8], ret[bad[:8]], want_ret[bad[:8]])
        bad = np.flatnonzero(reffix.fnv1a64_rows(list(out)) != want[:, 2])
        assert bad.size == 0, (t.name, bad[:8])
        if t.name.startswith("export"):
            for s in range(0, t.nsf, 5):
                rc, o = V.RScheckSuperframe(t.p[s], 0, t.rsdims, np.full(110 * t.rsdims, reffix.RS_SENTINEL, np.uint8))
                assert rc == int(want_ret[s]) and reffix.fnv1a64(o) == int(want[s, 2]), (t.name, s)
