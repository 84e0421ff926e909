"""CPU-only: the decision words of the oracle, the traceback models of tests/tbdirect.py and the committed merge-directed
set (tests/golden/tb_directed.json).  Non-vacuity of tests/test_gpu_tb_paths.py is asserted HERE, from the models alone:
which class of path every directed wave takes, how many distinct frames a class holds, how deep the cascades go.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import reffix  # noqa: E402
import tbdirect as D  # noqa: E402


@pytest.fixture(scope="module")
def census(O):
    have, deepest = D.census(O)  # asserts on the way that every model's bits are the serial chainback's
    print("traceback paths:", {c: len(v) for c, v in have.items()}, "deepest cascades:", deepest)
    return have, deepest


def test_decision_words_are_what_chainback_consumes(O):
    """a serial chainback in numpy over oracle.decisions() == oracle.decode_batch, every frame of the set, both comparators"""
    for sp in D.pinned_specs():
        sym = sp.symbols()
        for ge in (False, True):
            bits, _ = D.serial_chainback(O.decisions(sp.fb, sym, ge=ge), sp.fb)
            assert np.array_equal(D.pack_bits(bits), O.decode_batch(sp.fb, sym, ge=ge)[0]), (sp.key(), ge)


@pytest.mark.parametrize("ge", [False, True], ids=["gt150", "ge150"])
def test_numpy_acs_reproduces_the_decision_words(O, ge):
    """a plain numpy add-compare-select (no code shared with the oracle) gives the same words: soft, hard (renormalises
    often; the comparators differ) and directed short frames"""
    fams = [(fb, O.uniform_symbols(O.sym_len(fb), seed=fb + 3)) for fb in (2, 30, 200)]
    fams += [(fb, O.hard_random_symbols(1, fb, seed=1)[0]) for fb in (64, 400)] + [(fb, D.Spec(fb, 5, "hf").symbols()) for fb in (200, 400)]
    fams += [(sp.fb, sp.symbols()) for sp in D.pinned_specs() if sp.fb <= 304 and sp.bursts][:4]
    differ = 0
    for fb, sym in fams:
        assert np.array_equal(D.numpy_acs(sym, ge), O.decisions(fb, sym, ge=ge)), (fb, ge)
        differ += not np.array_equal(O.decisions(fb, sym, ge=False), O.decisions(fb, sym, ge=True))
    assert differ >= 3  # the comparator is exercised


def test_models_reach_chainback_on_every_frame_in_every_form(O):
    """every frame of the set also through the forms its own wave does not use: alone in a wave (general form, three
    empty slots), the latency kernel's form, four copies (fast form, after the forward pass and in flight) - and under the
    `>= 150` comparator.  A model that does not reach ChainBack is a bug in the model."""
    for sp in D.pinned_specs():
        for ge in (False, True):
            if ge and not (sp.db == "hf" or sp.bursts):
                continue
            f = D.make_frame(O, sp, ge)
            want = f.true()[0]
            assert np.array_equal(D.pack_bits(want), O.decode_batch(sp.fb, f.sym, ge=ge)[0])
            assert np.array_equal(D.general_wave([f, None, None, None]).bits[0], want), ("general", sp.key(), ge)
            assert np.array_equal(D.lat_wave(f).bits[0], want), ("lat", sp.key(), ge)
            if sp.fb % 16 == 0:
                for long_launch in (False, True):
                    w = D.packed_wave([f, f, f, f], long_launch)
                    assert w.form == ("inflight" if long_launch else "fast")
                    assert all(np.array_equal(b, want) for b in w.bits), (w.form, sp.key(), ge)


def test_every_class_is_populated(census):
    have, _ = census
    skipped = {c for c, _ in D.NOT_REACHED}
    for c in D.CLASSES:
        if c in skipped:
            continue
        need = 1 if c in D.ONE_EACH else D.NEED
        assert len(have[c]) >= need, "%s: %d distinct directed frames, %d needed" % (c, len(have[c]), need)
    # the two families the issue counts as one class each hold at least NEED frames together
    for prefix in ("fast.one_miss.lane", "fast.cascade"):
        assert len(set().union(*(have[c] for c in D.CLASSES if c.startswith(prefix)))) >= D.NEED
    # exactly 7 (keeps tracing) and exactly 8 (gives up), composed across the four frames in at least two ways
    for c in ("inflight.total7_keeps_tracing", "inflight.total8_gives_up"):
        ways = {tuple(sorted(k[-1].split("+"))) for k in have[c]}
        assert len(ways) >= 2, (c, ways)


def test_exclusion_list_is_short_and_never_a_required_class():
    assert len(D.NOT_REACHED) <= 3
    assert all(c in D.CLASSES and c not in D.REQUIRED and reason for c, reason in D.NOT_REACHED)
    assert set(D.REQUIRED) <= set(D.CLASSES)


def test_deepest_cascades(census):
    """recorded, and asserted so that a regenerated set cannot quietly become shallower: the fast form reaches 14, every
    speculative lane of a 16-lane part in a row (the most there is); the general form 11 of at most 15; the latency kernel
    30 of at most 63.  The kernels' pass bounds (17, 17, 65) leave room above each."""
    _, deepest = census
    assert deepest == {"fast": 14, "general": 11, "lat": 30}, deepest


def test_clean_companions_stay_out_of_the_way(O):
    """the noise-free frames that keep a directed frame company.  Noise-free is not miss-free: a speculative lane starts from
    state 0, and the best path INTO state 0 leaves the true one only gradually, so a lone block may miss (one does at 768
    bits).  What the classes rely on - they are evaluated on the whole wave's model, and the failing frame of a part is
    identified by its own positions - is only that companions never fail a check, never make a wave give up, never cascade."""
    for fb, long_launch in ((768, False), (400, False), (3072, True), (3200, True), (9216, True)):
        w = D.packed_wave([D.make_frame(O, D.clean_spec(fb, k)) for k in range(4)], long_launch)
        assert max(w.miss0.values()) <= 1 and max(max(d) for d in w.depth.values()) <= 1, fb
        assert not w.chain and w.gave_up_at is None and all(n <= 1 for n, _ in w.inflight_miss.values()), fb
    w = D.general_wave([D.make_frame(O, D.clean_spec(fb, k)) for k, fb in enumerate((778, 704, 582, 3070))])
    assert max(w.miss0.values()) <= 1 and not w.warm_switch


def test_the_search_is_reproducible(O):
    """the first stretch of the search (the composed miss totals, the 9216-bit waves, NP = 2 and 40 candidates of the
    single-segment family) again: the same waves, in the same order, as the head of the committed set"""
    kept, _, _ = D.search(O, limits=(("fast", 40),))
    kept = [w for w in kept if w.specs[w.directed].db != "hf"]
    committed, _ = D.load_directed()
    assert len(kept) >= 40
    assert [w.to_json() for w in kept] == [w.to_json() for w in committed[:len(kept)]]


def test_pinned_inputs_have_their_committed_digests():
    """the generators are seeded numpy: every frame rebuilt from its recipe has the digest recorded with the reference's results"""
    rows = np.load(D.TB_PATHS_NPY)
    specs = D.pinned_specs()
    assert rows.shape == (len(specs), len(D.PIN_COLS)) and rows.dtype == np.uint64
    assert np.array_equal(rows[:, 0], np.array([s.fb for s in specs], np.uint64))
    assert np.array_equal(reffix.fnv1a64_rows([s.symbols() for s in specs]), rows[:, 1])


def test_batches_cover_the_set():
    waves, _ = D.load_directed()
    bs = D.batches(waves)
    assert sum(len(b.waves) for b in bs) >= len(waves)
    assert {id(w) for b in bs for w in b.waves} >= {id(w) for w in waves}
    assert any(b.framebits == 9216 for b in bs) and any(b.framebits is None and b.long_launch for b in bs)
    assert any(b.framebits is None and not b.long_launch for b in bs)
