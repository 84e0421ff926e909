"""Generates tests/golden/reference_decoder.npy, reference_rs.npy and reference_provenance.json: RECORDED RESULTS OF THE
REFERENCE'S OWN CODE (oracle/_ref: its deconvolve.cpp and rschecksf.cpp, compiled in place - oracle/ref.py), on inputs
that tests/reffix.py rebuilds from seeds.  Needs oracle/_ref, i.e. a reference checkout at build time.

Decoder: per even framebits 2 ... 9216 the FNV-1a-64 of the output for a soft and a hard input family under
RENORMALIZE_THRESHOLD 150 (`> 150`, the C decoders as they are) and 149 (`>= 150`, the MASM decoders' comparator), plus
the digests of the inputs.  Every C variant this CPU runs (at 9216 bits: the 256-bit ones, see oracle/ref/harness.cpp) must produce the same bytes before anything is written.
RS: per seeded superframe the return value, the digest of the sentinel-initialised output, the digest of the input.
RS paths (reference_rs_paths.npy): the same four values for the syndrome-directed tables of tests/rsdirect.py
(pinned_tables(): 64 columns of every class on their own, the first-failure, wide and export tables).
Traceback paths (reference_tb_paths.npy): per merge-directed frame of tests/tbdirect.py (tests/golden/tb_directed.json) its
length, the digest of its symbols and the digests of the reference's output under both thresholds.

Arguments select the parts to (re)write - decoder, rs, rs_paths, tb_paths - default all; reference_provenance.json is updated
for the parts written.
"""
import datetime
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import _vitpkg  # noqa: E402
import reffix  # noqa: E402
import rsdirect  # noqa: E402
import tbdirect  # noqa: E402

ALL_PARTS = {"decoder", "rs", "rs_paths", "tb_paths"}
PARTS = set(sys.argv[1:]) or ALL_PARTS
assert PARTS <= ALL_PARTS, PARTS

R = _vitpkg.load_ref()
assert R.build(), "oracle/_ref is missing and there is no reference checkout to build it from"
variants = R.variants()
assert "sse2_lut32" in variants and len(variants) >= 4, variants

if "decoder" in PARTS:
    soft, hard = reffix.decoder_inputs()
    tab = np.zeros((len(reffix.LENGTHS), len(reffix.COLS)), np.uint64)
    tab[:, 0], tab[:, 1] = reffix.fnv1a64_rows(soft), reffix.fnv1a64_rows(hard)
    for col, fam, ge in ((2, soft, False), (3, soft, True), (4, hard, False), (5, hard, True)):
        outs = []
        for fb, sym in zip(reffix.LENGTHS, fam):
            got = [R.decode_batch(fb, sym, variant=v, ge=ge, nthreads=1)[0] for v in R.variants(fb)]
            assert all(np.array_equal(got[0], g) for g in got[1:]), ("the reference's variants disagree", fb, ge)
            outs.append(got[0])
        tab[:, col] = reffix.fnv1a64_rows(outs)
    np.save(reffix.DECODER_NPY, tab)

if "rs" in PARTS:
    rows = []
    for rsdims in reffix.RS_DIMS:
        p, _ = reffix.rs_superframes(rsdims)
        ret, out = R.rs_check_batch(p, rsdims, np.full((p.shape[0], 110 * rsdims), reffix.RS_SENTINEL, np.uint8))
        for s in range(p.shape[0]):
            rows.append((rsdims, int(ret[s]) & reffix.M64, reffix.fnv1a64(out[s]), reffix.fnv1a64(p[s])))
    np.save(reffix.RS_NPY, np.array(rows, np.uint64))

if "rs_paths" in PARTS:
    C = rsdirect.classes()
    ret_of = {label: R.rs_decode_words(k.words)[0] for label, k in C.items()}
    paths_counts = rsdirect.non_vacuity(ret_of)
    assert paths_counts["random_accepted"] >= 130, paths_counts  # of rsdirect.N_RANDOM columns: room above the tests' floor of 100
    paths = rsdirect.pinned_rows(R.rs_check_batch)
    np.save(rsdirect.RS_PATHS_NPY, paths)
    assert os.path.getsize(rsdirect.RS_PATHS_NPY) < os.path.getsize(os.path.join(HERE, "golden.json"))

if "tb_paths" in PARTS:
    def _ref_decode(fb, sym, ge):
        got = [R.decode_batch(fb, sym, variant=v, ge=ge, nthreads=1)[0] for v in R.variants(fb)]
        assert got and all(np.array_equal(got[0], g) for g in got[1:]), ("the reference's variants disagree", fb, ge)
        return got[0]
    tb = tbdirect.pinned_rows(_ref_decode, reffix.fnv1a64_rows)
    np.save(tbdirect.TB_PATHS_NPY, tb)

info = R.build_info()
prov = {}
if PARTS != ALL_PARTS:
    with open(reffix.PROVENANCE_JSON) as f:
        prov = json.load(f)
if PARTS & {"decoder", "rs"}:
    prov.update({"what": "outputs of the reference's own deconvolve.cpp / rschecksf.cpp (C decoders, -D_VIT_NO_ASM_), "
                         "built by oracle/ref.py with this repository's harness and stand-in headers",
                 "reference_tag": R.REFERENCE_TAG, "compiler": info.get("compiler"), "flags": info.get("flags"),
                 "thresholds": {"gt": 150, "ge": 149}, "variants_agreeing": variants,
                 "date": datetime.date.today().isoformat(),
                 "not_pinned": "the assembled MASM decoders; the GF tables of dllmain.cpp (the harness builds its own)"})
if "rs_paths" in PARTS:
    prov["rs_paths"] = {"what": "reference_rs_paths.npy: rschecksf.cpp on the syndrome-directed tables of tests/rsdirect.py",
                        "reference_tag": R.REFERENCE_TAG, "compiler": info.get("compiler"), "date": datetime.date.today().isoformat(),
                        "superframes": int(paths.shape[0]), "reference_counts": paths_counts,
                        "class_digests": rsdirect.class_digests()}
if "tb_paths" in PARTS:
    prov["tb_paths"] = {"what": "reference_tb_paths.npy: deconvolve.cpp (thresholds 150 and 149) on the merge-directed frames of "
                                "tests/tbdirect.py (tests/golden/tb_directed.json)",
                        "reference_tag": R.REFERENCE_TAG, "compiler": info.get("compiler"), "date": datetime.date.today().isoformat(),
                        "frames": int(tb.shape[0]), "variants_agreeing": variants,
                        "frames_on_which_the_thresholds_differ": int((tb[:, 2] != tb[:, 3]).sum())}
with open(reffix.PROVENANCE_JSON, "w") as f:
    json.dump(prov, f, indent=1)
print("wrote", sorted(PARTS), "variants", variants)
