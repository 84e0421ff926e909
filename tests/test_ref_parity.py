"""CPU-only: the oracle (oracle/vit_oracle.c, this repository's restatement) against a build of the REFERENCE'S OWN
decoders and RS checker (oracle/_ref, recipe: oracle/ref.py), and against the committed results of that build
(tests/golden/reference_*.npy, made by tests/golden/make_reference_golden.py).  Every comparison is of bytes and
return values and is exact.

The direct tests need oracle/_ref: where a reference checkout exists a missing build is made (a build failure is a test
failure), where neither exists they skip.  The fixture tests need neither and never skip.
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
import rsdirect  # noqa: E402
import tbdirect  # noqa: E402


@pytest.fixture(scope="module")
def R():
    mod = _vitpkg.load_ref()
    if mod.reference_dir() is None and not mod.available():
        pytest.skip("no oracle/_ref and no reference checkout to build it from ($VIT_REFERENCE_DIR or ../reference)")
    assert mod.build(), "oracle/_ref could not be built"
    v = mod.variants()
    assert "sse2_lut32" in v, v
    if O_has_avx2():
        assert len(v) >= 4 and "avx2" in v, v  # a variant is left out only for a CPU feature the host lacks
    return mod


def O_has_avx2():
    return _vitpkg.load_oracle().has_avx2()


def _all_agree(R, O, fb, sym, ge):
    """every variant of the reference build == every other == the oracle; returns the bytes"""
    want = O.decode_batch(fb, sym, nthreads=4, ge=ge)
    vs = R.variants(fb)
    assert vs and (fb > 9214 or "sse2_lut32" in vs), (fb, vs)
    for v in vs:
        got = R.decode_batch(fb, sym, variant=v, ge=ge)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, "framebits %d, variant %s, ge=%s: frames %s differ from the oracle" % (fb, v, ge, bad[:8])
    return want


def _stress(O, fb, n, seed):
    """the input of test_saturation_and_renorm_stress (tests/test_gpu_parity.py): metrics into the 255 clamp and the floor"""
    rng = np.random.default_rng(seed)
    sl = O.sym_len(fb)
    sym = np.empty((n, sl), np.uint8)
    sym[0::4], sym[1::4] = 0, 255
    sym[2::4] = rng.integers(0, 2, (n // 4, sl), dtype=np.uint8) * 255
    sym[3::4] = np.repeat(rng.integers(0, 256, (n // 4, sl // 64 + 1), dtype=np.uint8), 64, axis=1)[:, :sl]
    return sym


def _degenerate(O, fb):
    sl = O.sym_len(fb)
    alt = np.tile(np.array([0, 255], np.uint8), sl // 2)
    return np.stack([np.full(sl, v, np.uint8) for v in (0, 255, 127, 128)] + [alt, alt[::-1].copy()])


@pytest.mark.parametrize("ge", [False, True], ids=["gt150", "ge150"])
def test_every_even_length(R, O, ge):
    """every even framebits 2 ... 9216, a soft and a hard frame each (the fixture families): all variants == the oracle"""
    soft, hard = reffix.decoder_inputs()
    for fb, s, h in zip(reffix.LENGTHS, soft, hard):
        _all_agree(R, O, fb, np.stack([s, h]), ge)


@pytest.mark.parametrize("ge", [False, True], ids=["gt150", "ge150"])
@pytest.mark.parametrize("fb", [2, 96, 768, 778, 780, 1536, 3072, 3074, 6912, 9216])
def test_input_families(R, O, fb, ge):
    n = 24 if fb <= 3072 else 8
    fams = [O.noisy_frames(n, fb, seed=fb + 1, ebn0_db=db) for db in (5.0, 3.0, 1.0, -6.0)]  # -6 dB: far below threshold
    fams += [O.uniform_symbols(n * O.sym_len(fb), seed=fb + 2).reshape(n, -1), O.hard_random_symbols(n, fb, seed=fb + 3),
             O.hard_flipped_frames(n, fb, flip=0.2, seed=fb + 4), _stress(O, fb, 16, seed=fb + 5), _degenerate(O, fb)]
    _all_agree(R, O, fb, np.concatenate(fams), ge)


def test_large_batch_and_comparator_non_vacuity(R, O):
    """ten times the frame counts of test_renorm_comparator_ge_vs_gt, both comparators, every variant.  Non-vacuity on the
    REFERENCE'S outputs alone: the 149 and the 150 build differ on both hard-decision families in every length class
    (<= 778, 779 ... 3072, > 3072) and never on the soft families."""
    for fb, n in ((768, 1000), (3072, 600), (6912, 100)):
        soft = np.concatenate([O.noisy_frames(n // 2, fb, seed=3), O.uniform_symbols((n // 2) * O.sym_len(fb), seed=4).reshape(n // 2, -1)])
        _all_agree(R, O, fb, soft, False)
        _all_agree(R, O, fb, soft, True)
        assert np.array_equal(R.decode_batch(fb, soft), R.decode_batch(fb, soft, ge=True))
        for name, hard in (("random 0/255", O.hard_random_symbols(n, fb, seed=5)),
                           ("encoded, 20 % flips", O.hard_flipped_frames(n, fb, flip=0.2, seed=5))):
            _all_agree(R, O, fb, hard, False)
            _all_agree(R, O, fb, hard, True)
            differ = (R.decode_batch(fb, hard) != R.decode_batch(fb, hard, ge=True)).any(axis=1)
            assert differ.sum() >= 1, (fb, name)


@pytest.mark.parametrize("ge", [False, True], ids=["gt150", "ge150"])
def test_merge_directed_frames(R, O, ge):
    """every frame of the traceback-directed set (tests/tbdirect.py: erasure, near-erasure, uniform and hard bursts on
    noise-free, noisy and hard-decision bases): all variants == the oracle"""
    by_fb = {}
    for sp in tbdirect.pinned_specs():
        by_fb.setdefault(sp.fb, []).append(sp.symbols())
    assert len(by_fb) >= 20 and sum(len(v) for v in by_fb.values()) >= 200
    for fb, syms in by_fb.items():
        _all_agree(R, O, fb, np.stack(syms), ge)


@pytest.mark.parametrize("ge", [False, True], ids=["gt150", "ge150"])
def test_u32_entry_with_junk_above_the_low_byte(R, O, ge):
    """the reference ABI: one u32 per symbol.  Junk in the upper 24 bits, values > 255 in the low 9 bits: the LUT variant
    masks, the others truncate (deconvolve.cpp, note of 2024-09) - the same thing; all == oracle == the u8 path"""
    rng = np.random.default_rng(32)
    for fb in (2, 768, 770, 3072, 9216):
        low = O.uniform_symbols(O.sym_len(fb), seed=fb + 9)
        junk = rng.integers(0, 1 << 24, low.size, dtype=np.int64) << 8
        junk[::3] |= 0x100  # bit 8 set: > 255 within the low 9 bits
        s32 = (low.astype(np.int64) | junk).astype(np.uint32)
        assert (s32 & 0x1FF).max() > 255
        want = O.decode_batch(fb, low, ge=ge)[0]
        assert np.array_equal(O.deconvolve_u32(fb, s32, ge=ge), want)
        for v in R.variants(fb):
            assert np.array_equal(R.deconvolve_u32(fb, s32, variant=v, ge=ge), want), (fb, v)
            assert np.array_equal(R.deconvolve_u32(fb, s32, variant=v, ge=ge, dispatcher=True), want), (fb, v)
            assert np.array_equal(R.decode_batch(fb, low, variant=v, ge=ge)[0], want), (fb, v)


def test_harness_constants_from_the_polynomials(R):
    """the decoders' mask constants in the harness are data of the reference; here they follow from the code polynomials
    (109, 79, 83, 109) alone: an all-zero message, encoded, must decode to zeros and a random one to itself, per variant"""
    O = _vitpkg.load_oracle()
    rng = np.random.default_rng(7)
    for fb in (64, 768):
        bits = rng.integers(0, 2, fb, dtype=np.uint8)
        sym = (O.encode(bits) * 255).astype(np.uint8)
        for v in R.variants():
            assert np.array_equal(np.unpackbits(R.decode_batch(fb, sym, variant=v)[0]), bits), v
    ato, iof = R.tables()
    assert np.array_equal(ato, reffix.ALPHA[np.arange(768) % 255].astype(np.uint8))
    assert iof[0] == 255 and np.array_equal(iof[1:], reffix.LOG[1:].astype(np.uint8))


def test_128_bit_variants_stop_below_the_abi_maximum(R):
    """A finding about the reference, encoded as it behaves: at framebits == 9216 its 128-bit C decoders
    (sse2_lut32, ssse3, avx) write 2 bytes past their decision array - 4 * 2 * 4611 stores of 2 bytes each fill the
    9222 * 8 bytes exactly and every store is 4 bytes wide - so the harness refuses that one call; one length below, all
    variants run and agree; at 9216 the 256-bit variants (where the CPU has them) carry the comparison."""
    assert (4 * 2 * ((9216 + 6) // 2)) * 2 == (384 * 24 + 6) * 8
    assert set(R.variants(9216)) == set(R.variants()) - {"sse2_lut32", "ssse3", "avx"}
    assert R.variants(9214) == R.variants()
    sym = np.zeros(R.sym_len(9216), np.uint8)
    with pytest.raises(RuntimeError):
        R.decode_batch(9216, sym, variant="sse2_lut32")


# ---- RS ---------------------------------------------------------------------------------------------------------------

def test_rs_superframes_and_words(R, O):
    """about 10^5 columns over RSDims 1, 2, 7, 12, 24, 48 from the independent numpy encoder (tests/reffix.py): 0 ... 10
    errors per column, pure random columns, single symbols in the virtual padding, failures at the first / a middle / the
    last column; outputs start as a sentinel so that "left unwritten" is compared byte for byte."""
    seen = {"zero": 0, "positive": 0, "fail": 0, "padding_root": 0, "miscorrected": 0, "first": 0, "middle": 0, "last": 0}
    columns = 0
    for rsdims in reffix.RS_DIMS:
        nsf = 1100
        p, kind = reffix.rs_superframes(rsdims, nsf, salt=0x7E57)
        init = np.full((nsf, 110 * rsdims), reffix.RS_SENTINEL, np.uint8)
        ret, out = R.rs_check_batch(p, rsdims, init)
        ret_o, out_o = O.rs_check_batch(p, rsdims, init)
        assert np.array_equal(ret, ret_o), (rsdims, np.flatnonzero(ret != ret_o)[:8])
        assert np.array_equal(out, out_o), (rsdims, np.flatnonzero((out != out_o).any(axis=1))[:8])
        rc1, out1 = R.rs_check_superframe(p[1], rsdims, init[1].copy())  # the single call == the batch
        assert rc1 == ret[1] and np.array_equal(out1, out[1])
        columns += nsf * rsdims
        seen["zero"] += int((ret == 0).sum())
        seen["positive"] += int((ret > 0).sum())
        seen["fail"] += int((ret == -1).sum())
        # column by column: DECODE_RS on the full 120 symbols (the patched parity included)
        words = np.ascontiguousarray(p.reshape(nsf, 120, rsdims).transpose(0, 2, 1)).reshape(-1, 120)
        wret, wfix = R.rs_decode_words(words)
        k = kind.reshape(-1)
        seen["miscorrected"] += int(((k > 5) & (wret >= 0)).sum())
        padroot = (k == -2) & (wret == 1) & (wfix == words).all(axis=1)
        seen["padding_root"] += int(padroot.sum())
        for i in np.flatnonzero((k > 5) | (k < 0) | (np.arange(k.size) % 7 == 0)):  # the oracle has no batch call: a subset
            rc_o, fix_o = O.rs_decode_word(words[i])
            assert rc_o == wret[i] and np.array_equal(fix_o, wfix[i]), (rsdims, i, int(k[i]))
        if rsdims >= 7:
            untouched = (out.reshape(nsf, 110, rsdims) == reffix.RS_SENTINEL).all(axis=1)  # (nsf, rsdims)
            first_fail = np.where(ret == -1, untouched.argmax(axis=1), -1)
            assert (untouched[ret >= 0].sum() == 0)
            seen["first"] += int((first_fail == 0).sum())
            seen["middle"] += int((first_fail == rsdims // 2).sum())
            seen["last"] += int((first_fail == rsdims - 1).sum())
    print("RS: %d columns, %s" % (columns, seen))
    assert columns >= 100000
    assert all(v > 0 for v in seen.values()), seen


# ---- the committed vectors ---------------------------------------------------------------------------------------------

def test_reference_reproduces_golden_json(R):
    """tests/golden/golden.json was made by the oracle; the reference builds must give every out_hex (150), out_ge_hex
    (149), RS ret and RS out_hex in it"""
    import base64
    import zlib
    with open(os.path.join(reffix.GOLD, "golden.json")) as f:
        g = json.load(f)
    for case in g["decode"]:
        fb = case["framebits"]
        sym = np.frombuffer(zlib.decompress(base64.b64decode(case["sym_zb64"])), np.uint8)
        for v in R.variants(fb):
            assert R.decode_batch(fb, sym, variant=v)[0].tobytes().hex() == case["out_hex"], (fb, v)
            assert R.decode_batch(fb, sym, variant=v, ge=True)[0].tobytes().hex() == case["out_ge_hex"], (fb, v)
    for case in g["rs"]:
        p = np.frombuffer(bytes.fromhex(case["p_hex"]), np.uint8)
        rc, out = R.rs_check_superframe(p, case["rsdims"], np.full(110 * case["rsdims"], 0xA5, np.uint8))
        assert rc == case["ret"] and out.tobytes().hex() == case["out_hex"], case["note"]


def test_reference_build_reproduces_its_committed_fixtures(R):
    """the fixtures are what oracle/_ref computes today (a changed compiler or recipe shows here)"""
    tab = np.load(reffix.DECODER_NPY)
    lengths = reffix.LENGTHS[::37] + [768, 9216]
    soft, hard = reffix.decoder_inputs(lengths)
    for fb, s, h in zip(lengths, soft, hard):
        row = tab[reffix.LENGTHS.index(fb)]
        got = [reffix.fnv1a64(R.decode_batch(fb, x, ge=ge)[0]) for x in (s, h) for ge in (False, True)]
        assert got == [int(v) for v in row[2:]], fb
    rs = np.load(reffix.RS_NPY)
    rows = [(rsdims, int(r) & reffix.M64, reffix.fnv1a64(o), reffix.fnv1a64(p))
            for rsdims in reffix.RS_DIMS for P in [reffix.rs_superframes(rsdims)[0]]
            for p, r, o in zip(P, *R.rs_check_batch(P, rsdims, np.full((P.shape[0], 110 * rsdims), reffix.RS_SENTINEL, np.uint8)))]
    assert np.array_equal(np.array(rows, np.uint64), rs)
    assert np.array_equal(rsdirect.pinned_rows(R.rs_check_batch), np.load(rsdirect.RS_PATHS_NPY))  # the syndrome-directed tables
    tb = tbdirect.pinned_rows(lambda fb, sym, ge: R.decode_batch(fb, sym, ge=ge)[0], reffix.fnv1a64_rows)  # the merge-directed frames
    assert np.array_equal(tb, np.load(tbdirect.TB_PATHS_NPY))


def test_oracle_reproduces_the_reference_fixtures(O):
    """NEVER SKIPS: needs neither oracle/_ref nor a reference checkout.  The oracle reproduces every committed digest of the
    reference's outputs - 4608 lengths x {soft, hard} x {> 150, >= 150}, the merge-directed frames of tests/tbdirect.py -
    and every RS return value and output digest.
    The inputs are rebuilt from their seeds and checked against their own digests first."""
    tab = np.load(reffix.DECODER_NPY)
    assert tab.shape == (len(reffix.LENGTHS), len(reffix.COLS)) and tab.dtype == np.uint64
    soft, hard = reffix.decoder_inputs()
    assert np.array_equal(soft[383], O.uniform_symbols(O.sym_len(768), seed=reffix.soft_seed(768)))  # the C generator
    differ = 0
    for i, (fb, s, h) in enumerate(zip(reffix.LENGTHS, soft, hard)):
        assert O.fnv1a64(s) == int(tab[i, 0]) and O.fnv1a64(h) == int(tab[i, 1]), "input generator drifted at %d" % fb
        sym = np.stack([s, h])
        gt, ge = O.decode_batch(fb, sym), O.decode_batch(fb, sym, ge=True)
        got = [O.fnv1a64(gt[0]), O.fnv1a64(ge[0]), O.fnv1a64(gt[1]), O.fnv1a64(ge[1])]
        assert got == [int(v) for v in tab[i, 2:]], "framebits %d: oracle %s, reference %s" % (fb, got, tab[i, 2:])
        differ += got[2] != got[3]
    assert (tab[:, 2] == tab[:, 3]).all()  # soft input: the two comparators agree (as the reference behaves)
    assert differ > len(reffix.LENGTHS) // 10  # hard input: they do not
    rs = np.load(reffix.RS_NPY)
    assert rs.shape == (len(reffix.RS_DIMS) * reffix.RS_NSF, len(reffix.RS_COLS))
    row = 0
    for rsdims in reffix.RS_DIMS:
        p, _ = reffix.rs_superframes(rsdims)
        ret, out = O.rs_check_batch(p, rsdims, np.full((p.shape[0], 110 * rsdims), reffix.RS_SENTINEL, np.uint8))
        for s in range(p.shape[0]):
            want = rs[row]
            assert int(want[0]) == rsdims and O.fnv1a64(p[s]) == int(want[3]), "RS input generator drifted"
            assert (int(ret[s]) & reffix.M64) == int(want[1]) and O.fnv1a64(out[s]) == int(want[2]), (rsdims, s)
            row += 1
    rets = np.ascontiguousarray(rs[:, 1]).view(np.int64)
    assert (rets == 0).any() and (rets > 0).any() and (rets == -1).any()
    # the syndrome-directed tables (tests/rsdirect.py): every return value, output digest and input digest
    paths = np.load(rsdirect.RS_PATHS_NPY)
    got = rsdirect.pinned_rows(O.rs_check_batch)
    assert got.shape == paths.shape and np.array_equal(got[:, 3], paths[:, 3]), "RS path generator drifted"
    assert np.array_equal(got, paths), np.flatnonzero((got != paths).any(axis=1))[:8]
    prets = np.ascontiguousarray(paths[:, 1]).view(np.int64)
    assert (paths[:, 0] == 1).sum() >= 64 * 48 and (prets[paths[:, 0] == 1] == 6).sum() >= 64  # degree-6 locators, accepted
    # the merge-directed frames (tests/tbdirect.py): input digests, then the output digests under both comparators
    tb = np.load(tbdirect.TB_PATHS_NPY)
    got = tbdirect.pinned_rows(lambda fb, sym, ge: O.decode_batch(fb, sym, ge=ge)[0], reffix.fnv1a64_rows)
    assert got.shape == tb.shape and np.array_equal(got[:, :2], tb[:, :2]), "traceback path generator drifted"
    assert np.array_equal(got, tb), np.flatnonzero((got != tb).any(axis=1))[:8]
    assert (tb[:, 2] != tb[:, 3]).sum() >= 9  # the hard-decision bases: the comparators decode them differently
    with open(reffix.PROVENANCE_JSON) as f:
        prov = json.load(f)
    assert prov["reference_tag"] == "2024_10_08"
    assert prov["tb_paths"]["frames"] == tb.shape[0]
