"""CPU-only: puncturing profiles (include/viterbi_amd.h vit_punct_profile) - vit_punctured_length, the Python
profile builder's bit order, the export table - and the numpy depuncturer the GPU tests use as their reference
(tests/test_gpu_punctured.py applies it before the oracle's decoder)."""
import subprocess

import numpy as np
import pytest

TAIL = 6


# ---- numpy reference ------------------------------------------------------------------------------------------------

def keep_mask(segments, framebits=None):
    """bool array of 4 symbols per step (= 4*(framebits+6), checked when framebits is given): True = transmitted.
    Segment k's pattern period restarts at its own first step; bit 4*(k mod 8) + j of keep = symbol j of the
    segment's k-th step."""
    parts = []
    for steps, keep in segments:
        k = np.arange(steps)
        bits = 4 * (k[:, None] % 8) + np.arange(4)[None, :]
        parts.append(((int(keep) >> bits) & 1).astype(bool).reshape(-1))
    m = np.concatenate(parts) if parts else np.zeros(0, bool)
    assert framebits is None or m.size == 4 * (framebits + TAIL), "profile does not cover framebits + 6 steps"
    return m


def puncture(sym, segments, framebits=None):
    """(nframes, 4*(framebits+6)) soft symbols -> (nframes, P) transmitted symbols"""
    m = keep_mask(segments, framebits)
    sym = np.asarray(sym, np.uint8).reshape(-1, m.size)
    return np.ascontiguousarray(sym[:, m])


def depuncture(punct, segments, framebits=None, erasure=128):
    """(nframes, P) transmitted symbols -> (nframes, 4*(framebits+6)), the punctured positions set to `erasure`"""
    m = keep_mask(segments, framebits)
    punct = np.asarray(punct, np.uint8)
    punct = punct.reshape(-1 if punct.size else len(punct), int(m.sum()))  # (P may be 0)
    out = np.full((punct.shape[0], m.size), erasure, np.uint8)
    out[:, m] = punct
    return out


def vec(s):
    """a puncturing vector v0...v31 as a keep mask"""
    return sum(1 << i for i, v in enumerate(s) if v == "1")


# FIC-shaped masks (EN 300 401 clause 11 gives the real vectors; these have the same weights): every step keeps
# symbols 0 and 1 (generators 133 and 171 octal), so the noise-free decode is unique
KEEP_24 = vec("1110" * 8)               # 24 of 32: symbols 0, 1, 2 of every step
KEEP_23 = vec("1110" * 7 + "1100")      # 23 of 32
KEEP_TAIL_12 = vec("1100" * 6)          # 12 of the 24 tail bits


def fic_segments():
    """768 bits: 21 blocks of 128 bits (32 steps each) under a 24-of-32 vector, 3 under a 23-of-32 vector, the tail"""
    return [(21 * 32, KEEP_24), (3 * 32, KEEP_23), (6, KEEP_TAIL_12)]


# ---- tests ----------------------------------------------------------------------------------------------------------

def test_numpy_depuncturer_hand_example():
    # a 2-step profile: keep 0b0110_1001 -> step 0 keeps symbols 0 and 3, step 1 keeps symbols 1 and 2
    segs = [(2, 0b01101001)]
    m = keep_mask(segs)
    assert m.tolist() == [True, False, False, True, False, True, True, False]
    punct = np.array([[10, 13, 21, 22]], np.uint8)
    assert depuncture(punct, segs, erasure=128).tolist() == [[10, 128, 128, 13, 128, 21, 22, 128]]
    sym = np.array([[10, 11, 12, 13, 20, 21, 22, 23]], np.uint8)
    assert puncture(sym, segs).tolist() == [[10, 13, 21, 22]]
    # two segments: the second one's pattern period restarts at its own first step
    segs = [(1, 0xF), (1, 0x1)]
    assert keep_mask(segs).tolist() == [True] * 4 + [True, False, False, False]


def test_all_ones_profile_is_the_unpunctured_length(V):
    for fb in (0, 2, 288, 768, 778, 9216):
        assert V.punctured_length([(fb + TAIL, 0xFFFFFFFF)], fb) == 4 * (fb + TAIL)
        assert V.punctured_length([(fb + 1, 0xFFFFFFFF), (5, 0xFFFFFFFF)], fb) == 4 * (fb + TAIL)


def test_fic_shape_gives_2304(V):
    segs = fic_segments()
    assert bin(KEEP_24).count("1") == 24 and bin(KEEP_23).count("1") == 23 and bin(KEEP_TAIL_12).count("1") == 12
    assert V.punctured_length(segs, 768) == 2304 == int(keep_mask(segs, 768).sum())
    # other masks of the same weights give the same length
    rng = np.random.default_rng(1)
    for _ in range(5):
        k24, k23, kt = (int(sum(1 << int(b) for b in rng.choice(n, w, replace=False))) for n, w in ((32, 24), (32, 23), (24, 12)))
        assert V.punctured_length([(672, k24), (96, k23), (6, kt)], 768) == 2304


def test_segment_ending_mid_period(V):
    rng = np.random.default_rng(7)
    for _ in range(200):
        fb = 2 * int(rng.integers(0, 200))
        T = fb + TAIL
        nseg = int(rng.integers(1, 9))
        if nseg > T:
            nseg = T
        cuts = np.sort(rng.choice(np.arange(1, T), nseg - 1, replace=False)) if nseg > 1 else np.array([], int)
        steps = np.diff(np.concatenate(([0], cuts, [T])))
        segs = [(int(s), int(rng.integers(0, 1 << 32))) for s in steps]
        assert V.punctured_length(segs, fb) == int(keep_mask(segs, fb).sum()), segs
    # by hand: 14 steps = one full period (5 ones) + 6 steps, whose bits 0..23 hold 4 of them
    keep = (1 << 0) | (1 << 6) | (1 << 17) | (1 << 20) | (1 << 31)
    assert V.punctured_length([(14, keep)], 8) == 5 + 4


def test_invalid_profiles_give_minus_one(V):
    assert V.punctured_length([(773, 0xFFFFFFFF)], 768) == -1     # one step short
    assert V.punctured_length([(775, 0xFFFFFFFF)], 768) == -1     # one step long
    assert V.punctured_length([(774, 0xFFFFFFFF), (0, 0xFF)], 768) == -1  # a segment of zero steps
    assert V.punctured_length([(0, 0xFF), (774, 0xFFFFFFFF)], 768) == -1
    p = V.PunctProfile()
    p.nsegs = 0
    assert V.punctured_length(p, 768) == -1
    p = V.punct_profile([(86, 0xFFFFFFFF)] * 8)
    assert V.punctured_length(p, 682) == 4 * 688                  # 8 segments: the maximum
    p.nsegs = 9                                                    # more than VIT_PUNCT_MAX_SEGS
    assert V.punctured_length(p, 682) == -1
    # steps whose 32-bit sum would wrap around to framebits + 6
    assert V.punctured_length([(0xFFFFFFFF, 1), (775, 1)], 768) == -1
    assert V.lib().vit_punctured_length(None, 768) == -1
    with pytest.raises(ValueError):
        V.punct_profile([(1, 1)] * 9)


def test_punct_profile_bit_order(V):
    s = "1" + "0" * 31
    assert V.punct_profile([(8, s)]).seg[0].keep == 1
    s = "0" * 31 + "1"
    assert V.punct_profile([(8, s)]).seg[0].keep == 1 << 31
    rng = np.random.default_rng(3)
    for _ in range(20):
        bits = rng.integers(0, 2, 32)
        s = "".join(str(b) for b in bits)
        p = V.punct_profile([(8, s), (4, int(vec(s)))])
        assert p.seg[0].keep == p.seg[1].keep == sum(int(b) << i for i, b in enumerate(bits))
        assert p.nsegs == 2 and p.seg[0].steps == 8 and p.seg[1].steps == 4
    assert V.punct_profile([(6, "1100" * 6)]).seg[0].keep == KEEP_TAIL_12  # a 24-bit tail vector
    with pytest.raises(ValueError):
        V.punct_profile([(8, "10x1")])
    import ctypes as C
    assert C.sizeof(V.PunctProfile) == 68
    img = V.profiles_bytes([fic_segments(), [(774, 0xFFFFFFFF)]])
    assert img.size == 136 and img[:4].view("<u4")[0] == 3 and img[4:8].view("<u4")[0] == 672
    assert img[68 + 8:68 + 12].view("<u4")[0] == 0xFFFFFFFF


def test_punctured_exports(V):
    out = subprocess.check_output(["nm", "-D", "--defined-only", V.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in ("vit_punctured_length", "vit_decode_punctured_dev", "vit_decode_punctured_varlen_dev"):
        assert name in exported and name in V.EXPORTS


def test_punctured_calls_fail_loudly(V):
    """without a device: VIT_ERR_NO_DEVICE; with one, null buffers are VIT_ERR_ARG - nothing is launched either way"""
    import ctypes as C
    import torch
    want = 1 if torch.cuda.is_available() else 2  # VIT_ERR_ARG / VIT_ERR_NO_DEVICE
    p = V.punct_profile(fic_segments())
    assert V.lib().vit_decode_punctured_dev(None, None, 768, 4, C.byref(p), 128, None) == want
    assert V.lib().vit_decode_punctured_varlen_dev(None, 0, None, 0, None, 4, 768, None, 1, 128, None) == want
    if want == 2:
        assert "gfx950" in V.last_error()
    assert V.punctured_length(p, 768) == 2304  # the host helper needs no GPU
