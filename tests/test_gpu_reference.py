"""GPU: the HIP kernels against the COMMITTED RESULTS OF THE REFERENCE'S OWN CODE (tests/golden/reference_*.npy, made by
tests/golden/make_reference_golden.py from a build of the reference's deconvolve.cpp / rschecksf.cpp).  Reads only the
fixtures and the seeded inputs of tests/reffix.py: no oracle, no oracle/_ref, no reference checkout.  Exact: a digest
of every output.
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
import tbdirect  # noqa: E402

GE_COL = {0: (2, 4), 1: (3, 5)}  # renorm_ge -> (column of the soft family, column of the hard family)


@pytest.fixture(scope="module")
def fix():
    """inputs rebuilt from their seeds and checked against their committed digests: a drifting generator fails here"""
    tab = np.load(reffix.DECODER_NPY)
    assert tab.shape == (len(reffix.LENGTHS), len(reffix.COLS))
    soft, hard = reffix.decoder_inputs()
    assert np.array_equal(reffix.fnv1a64_rows(soft), tab[:, 0]) and np.array_equal(reffix.fnv1a64_rows(hard), tab[:, 1])
    return tab, soft, hard


def _table_digests(V, torch, frames, fbs, kernel, ge):
    """one variable-length launch over all frames -> FNV-1a-64 of every frame's output"""
    desc, sym_bytes, out_bytes = V.make_descs(fbs)
    d_sym = torch.from_numpy(np.concatenate(frames)).cuda()
    d_desc = torch.from_numpy(desc.view(np.uint8)).cuda()
    d_out = torch.full((out_bytes,), 0xEE, dtype=torch.uint8, device="cuda")
    old, old_ge = V.set_kernel(kernel), V.set_renorm_ge(ge)
    try:
        V.decode_varlen_dev(d_sym, d_out, d_desc, len(fbs), max(fbs))
        torch.cuda.synchronize()
    finally:
        V.set_renorm_ge(old_ge)
        V.set_kernel(old)
    got = d_out.cpu().numpy()
    oo = desc["out_offset"].astype(np.int64)
    return reffix.fnv1a64_rows([got[o:o + (fb + 7) // 8] for o, fb in zip(oo, fbs)])


def _check(dig, tab, idx, ge, what):
    n = len(idx)
    want = np.concatenate([tab[idx, GE_COL[ge][0]], tab[idx, GE_COL[ge][1]]])
    bad = np.flatnonzero(dig != want)
    assert bad.size == 0, "%s: %d frames differ from the reference, first (framebits, family): %s" % (
        what, bad.size, [(reffix.LENGTHS[idx[b % n]], "soft" if b < n else "hard") for b in bad[:6]])


@pytest.mark.parametrize("ge", [0, 1], ids=["gt150", "ge150"])
@pytest.mark.parametrize("kernel", [0, 1, 2, 3])
def test_every_length_in_one_table(V, torch_cuda, fix, kernel, ge):
    """every product kernel (and the automatic choice) under both comparators: one descriptor table of all 4608 even
    lengths x {soft, hard} must reproduce every digest of the reference's output"""
    tab, soft, hard = fix
    idx = list(range(len(reffix.LENGTHS)))
    dig = _table_digests(V, torch_cuda, soft + hard, reffix.LENGTHS * 2, kernel, ge)
    _check(dig, tab, idx, ge, "kernel %d ge %d" % (kernel, ge))


# a subset that reaches every traceback form (the length lists of tests/test_gpu_parity.py): one segment (<= 778), the
# straight-line form (multiples of 16), the in-flight parts (784, 1008, 1040, 3072), the longest DAB frame and the ABI's maximum
UNIFORM = [2, 8, 96, 288, 768, 770, 778, 16, 1600, 2048, 784, 1008, 1040, 3072, 6912, 9216]


@pytest.mark.parametrize("ge", [0, 1], ids=["gt150", "ge150"])
@pytest.mark.parametrize("kernel", [0, 1, 2, 3])
def test_uniform_length_entry(V, torch_cuda, fix, kernel, ge):
    """vit_decode_batch_dev: eight frames per length ([soft, hard] x 4: whole groups of four equally long frames)"""
    torch = torch_cuda
    tab, soft, hard = fix
    old, old_ge = V.set_kernel(kernel), V.set_renorm_ge(ge)
    try:
        for fb in UNIFORM:
            i = reffix.LENGTHS.index(fb)
            sym = np.stack([soft[i], hard[i]] * 4)
            d_out = torch.full((8, (fb + 7) // 8), 0xEE, dtype=torch.uint8, device="cuda")
            V.decode_batch_dev(torch.from_numpy(sym).cuda(), d_out, fb, 8)
            torch.cuda.synchronize()
            dig = reffix.fnv1a64_rows(list(d_out.cpu().numpy()))
            want = np.array([tab[i, GE_COL[ge][0]], tab[i, GE_COL[ge][1]]] * 4, np.uint64)
            assert np.array_equal(dig, want), (fb, kernel, ge)
            if kernel == 0:  # the drop-in export, reference ABI (u32 symbols)
                rc, one = V.deconvolve(fb, hard[i].astype(np.uint32))
                assert rc == 0 and reffix.fnv1a64(one) == int(tab[i, GE_COL[ge][1]]), (fb, ge)
    finally:
        V.set_renorm_ge(old_ge)
        V.set_kernel(old)


@pytest.mark.parametrize("ge", [0, 1], ids=["gt150", "ge150"])
@pytest.mark.parametrize("kernel", [0, 1, 2, 3])
def test_merge_directed_frames(V, torch_cuda, kernel, ge):
    """the traceback-directed set of tests/tbdirect.py (every path of the block-parallel tracebacks: tests/test_tb_paths_host.py)
    against the recorded outputs of the reference's decoders, no oracle: one descriptor table of all frames, and the
    uniform-length entry per length in whole waves"""
    torch = torch_cuda
    rows = np.load(tbdirect.TB_PATHS_NPY)
    specs = tbdirect.pinned_specs()
    syms = [s.symbols() for s in specs]
    assert rows.shape == (len(specs), len(tbdirect.PIN_COLS))
    assert np.array_equal(reffix.fnv1a64_rows(syms), rows[:, 1]), "traceback path generator drifted"
    want = rows[:, 3 if ge else 2]
    fbs = [s.fb for s in specs]
    dig = _table_digests(V, torch, syms, fbs, kernel, ge)
    bad = np.flatnonzero(dig != want)
    assert bad.size == 0, "kernel %d ge %d: %d frames differ from the reference, first recipes: %s" % (
        kernel, ge, bad.size, [specs[b].key() for b in bad[:4]])
    old, old_ge = V.set_kernel(kernel), V.set_renorm_ge(ge)
    try:
        for fb in sorted(set(fbs)):
            idx = [i for i, f in enumerate(fbs) if f == fb]
            idx = (idx * 4)[:max(4, len(idx) // 4 * 4)]  # whole groups of four equally long frames
            d_out = torch.full((len(idx), (fb + 7) // 8), 0xEE, dtype=torch.uint8, device="cuda")
            V.decode_batch_dev(torch.from_numpy(np.stack([syms[i] for i in idx])).cuda(), d_out, fb, len(idx))
            torch.cuda.synchronize()
            assert np.array_equal(reffix.fnv1a64_rows(list(d_out.cpu().numpy())), want[idx]), (fb, kernel, ge)
    finally:
        V.set_renorm_ge(old_ge)
        V.set_kernel(old)


@pytest.mark.parametrize("ge", [0, 1], ids=["gt150", "ge150"])
def test_pk8_experiment_kernel(V, torch_cuda, fix, ge):
    """the 8-frames-per-wavefront experiment (one segment: <= 778 bits), only in a build that has it (tests/test_gpu_pk8.py)"""
    old = V.set_kernel(4)
    have = V.set_kernel(old) == 4
    if not have:
        pytest.skip("libviterbi.so was built without -DVIT_WITH_PK8 (the 8-frames-per-wavefront experiment)")
    tab, soft, hard = fix
    idx = [i for i, fb in enumerate(reffix.LENGTHS) if fb <= 778]
    dig = _table_digests(V, torch_cuda, [soft[i] for i in idx] + [hard[i] for i in idx], [reffix.LENGTHS[i] for i in idx] * 2, 4, ge)
    _check(dig, tab, idx, ge, "pk8 ge %d" % ge)


def test_rs_batch_and_export(V, torch_cuda):
    """vit_rs_batch_dev and the RScheckSuperframe export against the reference's return values and output digests
    (outputs start as the sentinel: columns the reference leaves unwritten must stay untouched)"""
    torch = torch_cuda
    rs = np.load(reffix.RS_NPY)
    assert rs.shape == (len(reffix.RS_DIMS) * reffix.RS_NSF, len(reffix.RS_COLS))
    row = 0
    for rsdims in reffix.RS_DIMS:
        p, _ = reffix.rs_superframes(rsdims)
        nsf = p.shape[0]
        want = rs[row:row + nsf]
        row += nsf
        assert (want[:, 0] == rsdims).all()
        assert [reffix.fnv1a64(x) for x in p] == [int(v) for v in want[:, 3]], "RS input generator drifted"
        want_ret = np.ascontiguousarray(want[:, 1]).view(np.int64)
        d_out = torch.full((nsf, 110 * rsdims), reffix.RS_SENTINEL, dtype=torch.uint8, device="cuda")
        d_ret = torch.full((nsf,), 12345, dtype=torch.int32, device="cuda")
        V.rs_batch_dev(torch.from_numpy(p).cuda(), d_out, d_ret, rsdims, nsf)
        torch.cuda.synchronize()
        assert np.array_equal(d_ret.cpu().numpy().astype(np.int64), want_ret), rsdims
        assert [reffix.fnv1a64(x) for x in d_out.cpu().numpy()] == [int(v) for v in want[:, 2]], rsdims
        for s in range(nsf):
            rc, out = V.RScheckSuperframe(p[s], 0, rsdims, np.full(110 * rsdims, reffix.RS_SENTINEL, np.uint8))
            assert rc == int(want_ret[s]) and reffix.fnv1a64(out) == int(want[s, 2]), (rsdims, s)
