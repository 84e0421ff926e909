"""The decision-history layout of the packed kernels (csrc/vit_pk.hip: acs_step): a step's decision is one v_bfi from the packed
difference m0 - m1 at a bit position 8..15 of its half, with ONE `>> 8` per 16-step block.  It can go wrong only where bit 8 of
a difference is not its sign, or at the shift points; tests/hist_layout_cases.py keeps frames that put differences of both
signs and a magnitude >= 128 (bit 7 != bit 8) there.

CPU half: the numpy trellis of the helper module IS the oracle's (decision words equal), no difference leaves [-255, 255],
and the directed set of every length contains what its docstring lists - for m0 - m1 and m2 - m3, both signs, at
block-relative steps 0, 7, 8 and 15 and in the six-step last block of 768 and 784.  That list is narrowed for the two shortest
lengths, by the trellis and not by any decoder: the metrics start 63 apart, so |d| <= 126 at step 0 and a difference of
magnitude >= 128 at block-relative step 0 needs a second block; 2 bits (T = 8) has steps 0..7 only, so position 7 is all it is
asked for, and 10 bits (T = 16) positions 7, 8 and 15.  From 26 bits (T = 32) on all four are required.  The
largest magnitude the directed frames reach at those places is 162 at 2 bits (T = 8: the metrics have had seven steps to spread),
189 at 10, 255 at 26, 170 at 762, 161 at 768 and 174 at 784 bits (printed by the test; the 255 clamp bounds it).

GPU half: those frames, each in each of the four slots of a wave, through kernels 1 (cross-check), 2 (packed) and auto, the
uniform entry and descriptor tables, both comparators, framebits 2, 10, 26, 762, 768 and 784 - byte for byte against the
oracle; the 768-bit launches once more in a child process on libviterbi_general.so.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import hist_layout_cases as H  # noqa: E402


# ---- CPU half ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", H.FRAMEBITS)
def test_numpy_trellis_is_the_oracles(O, fb):
    sym = H.directed(fb)[0]
    for ge in (False, True):
        d01, d23, dec = H.acs(sym, ge=ge)
        for k in range(sym.shape[0]):
            assert np.array_equal(dec[k], O.decisions(fb, sym[k], ge=ge)), (fb, k, ge)
        # what the eight-position insert rests on: bits 8..15 of a difference are copies of its sign
        assert max(int(np.abs(d01).max()), int(np.abs(d23).max())) <= 255


@pytest.mark.parametrize("fb", H.FRAMEBITS)
def test_directed_set_reaches_the_layouts_edges(fb):
    sym, met, big = H.directed(fb)
    need = H.requirements(fb)
    print("fb=%d: %d directed frames, %d requirements, largest |d| = %d" % (fb, sym.shape[0], len(need), big))
    assert sorted(met) == sorted(need), "not reached: %s" % sorted(set(need) - set(met))
    assert big >= 128
    # the lengths have the positions the issue names
    want_pos = {2: (7,), 10: (7, 8, 15)}.get(fb, (0, 7, 8, 15))
    assert H.reachable_positions(fb) == want_pos
    assert H.has_last6(fb) == (fb in (768, 784))
    assert sym.shape[0] <= 8, "a few frames per length: the batch stays small"


def test_batch_puts_every_directed_frame_in_every_slot():
    fb = 768
    sym, b = H.directed(fb)[0], H.batch(fb)
    assert b.shape == (16 * sym.shape[0], H.reffix.sym_len(fb))
    for k in range(sym.shape[0]):
        hits = [i % 4 for i in range(16 * k, 16 * k + 16) if np.array_equal(b[i], sym[k])]
        assert hits == [0, 1, 2, 3]


# ---- GPU half ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def data(O):
    return H.Data(O)


@pytest.mark.gpu
@pytest.mark.parametrize("ge", [0, 1], ids=["gt150", "ge150"])
@pytest.mark.parametrize("fb", H.FRAMEBITS)
def test_hist_layout(V, torch_cuda, data, fb, ge):
    msgs = [m for m in H.case(V, torch_cuda, data, fb, ge) if m]
    assert not msgs, "\n".join(msgs)


@pytest.mark.gpu
def test_768_without_the_fixed_instantiation(V, torch_cuda):
    """libviterbi_general.so (-DVIT_FIC_FIXED=0) in a fresh process: the 768-bit launches on the general kernel"""
    lib = os.path.join(os.path.dirname(V.LIB_PATH), "libviterbi_general.so")
    assert os.path.exists(lib), "libviterbi_general.so is missing: __graft_entry__.build() makes it"
    env = dict(os.environ, VITERBI_AMD_LIB=lib)
    r = subprocess.run([sys.executable, os.path.join(HERE, "hist_layout_cases.py")], env=env, capture_output=True, text=True, timeout=300)
    lines = r.stdout.splitlines()
    bad = [ln for ln in lines if not ln.startswith("ok ")]
    assert r.returncode == 0 and not bad and len(lines) == 2, "%s\n%s" % ("\n".join(bad[:8] or lines[-8:]), r.stderr[-2000:])
