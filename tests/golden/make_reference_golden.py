"""Generates tests/golden/reference_decoder.npy, reference_rs.npy and reference_provenance.json: RECORDED RESULTS OF THE
REFERENCE'S OWN CODE (oracle/_ref: its deconvolve.cpp and rschecksf.cpp, compiled in place - oracle/ref.py), on inputs
that tests/reffix.py rebuilds from seeds.  Needs oracle/_ref, i.e. a reference checkout at build time.

Decoder: per even framebits 2 ... 9216 the FNV-1a-64 of the output for a soft and a hard input family under
RENORMALIZE_THRESHOLD 150 (`> 150`, the C decoders as they are) and 149 (`>= 150`, the MASM decoders' comparator), plus
the digests of the inputs.  Every C variant this CPU runs (at 9216 bits: the 256-bit ones, see oracle/ref/harness.cpp) must produce the same bytes before anything is written.
RS: per seeded superframe the return value, the digest of the sentinel-initialised output, the digest of the input.
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

R = _vitpkg.load_ref()
assert R.build(), "oracle/_ref is missing and there is no reference checkout to build it from"
variants = R.variants()
assert "sse2_lut32" in variants and len(variants) >= 4, variants

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

rows = []
for rsdims in reffix.RS_DIMS:
    p, _ = reffix.rs_superframes(rsdims)
    ret, out = R.rs_check_batch(p, rsdims, np.full((p.shape[0], 110 * rsdims), reffix.RS_SENTINEL, np.uint8))
    for s in range(p.shape[0]):
        rows.append((rsdims, int(ret[s]) & reffix.M64, reffix.fnv1a64(out[s]), reffix.fnv1a64(p[s])))
np.save(reffix.RS_NPY, np.array(rows, np.uint64))

info = R.build_info()
with open(reffix.PROVENANCE_JSON, "w") as f:
    json.dump({"what": "outputs of the reference's own deconvolve.cpp / rschecksf.cpp (C decoders, -D_VIT_NO_ASM_), "
                       "built by oracle/ref.py with this repository's harness and stand-in headers",
               "reference_tag": R.REFERENCE_TAG, "compiler": info.get("compiler"), "flags": info.get("flags"),
               "thresholds": {"gt": 150, "ge": 149}, "variants_agreeing": variants,
               "date": datetime.date.today().isoformat(),
               "not_pinned": "the assembled MASM decoders; the GF tables of dllmain.cpp (the harness builds its own)"},
              f, indent=1)
print("wrote", reffix.DECODER_NPY, tab.shape, "and", reffix.RS_NPY, len(rows), "superframes; variants", variants)
