"""CPU-only: the three definitions after the decoder (include/viterbi_amd.h, "After the decoder") as numpy / integer
models independent of the library - the energy dispersal PRBS, the FIB CRC-16 and the DAB+ fire code - pinned by
their published properties, and the library's host PRBS checked against the model.  tests/test_gpu_dab.py uses the
same models as its reference."""
import ctypes as C
import subprocess

import numpy as np
import pytest

MAX_FRAMEBITS = 9216


# ---- energy dispersal PRBS: p_i = p_{i-9} ^ p_{i-5}, p_{-9} ... p_{-1} = 1 -------------------------------------------

def prbs_bits(n):
    p = [1] * 9  # p_{-9} ... p_{-1}
    for i in range(n):
        p.append(p[i] ^ p[i + 4])  # p_{i-9} ^ p_{i-5}
    return np.array(p[9:], np.uint8)


_PRBS = prbs_bits(MAX_FRAMEBITS)


def prbs_bytes_model(framebits):
    """the PRBS as the XOR bytes of one frame, MSB first, padding bits 0"""
    bits = np.zeros(8 * ((framebits + 7) // 8), np.uint8)
    bits[:framebits] = _PRBS[:framebits]
    return np.packbits(bits)


def scramble(frames, framebits):
    """(nframes, (framebits+7)//8) bytes XOR the PRBS on the valid bits (self-inverse)"""
    frames = np.asarray(frames, np.uint8)
    return frames ^ prbs_bytes_model(framebits)[None, :]


# ---- FIB CRC: CRC-16/GENIBUS (0x1021, preset 0xFFFF, MSB first, ones' complement) -------------------------------------

def crc16_genibus(data):
    r = 0xFFFF
    for byte in bytes(data):
        for k in range(7, -1, -1):
            fb = ((r >> 15) ^ (byte >> k)) & 1
            r = (r << 1) & 0xFFFF
            if fb:
                r ^= 0x1021
    return r ^ 0xFFFF


def make_fib(payload30):
    c = crc16_genibus(payload30)
    return np.concatenate([np.asarray(payload30, np.uint8), np.array([c >> 8, c & 0xFF], np.uint8)])


def fib_ok_model(fibs):
    """(n, 32) descrambled FIBs -> n flags"""
    fibs = np.asarray(fibs, np.uint8).reshape(-1, 32)
    return np.array([crc16_genibus(f[:30]) == (int(f[30]) << 8 | int(f[31])) for f in fibs], np.uint8)


# ---- DAB+ fire code: GF(2) polynomials as Python ints, bit k = coefficient of x^k -----------------------------------

FIRE_F1 = (1 << 11) | 1                                      # x^11 + 1
FIRE_F2 = (1 << 5) | (1 << 3) | (1 << 2) | (1 << 1) | 1      # x^5 + x^3 + x^2 + x + 1


def pmul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a <<= 1
        b >>= 1
    return r


def pmod(a, g):
    dg = g.bit_length() - 1
    while a and a.bit_length() - 1 >= dg:
        a ^= g << (a.bit_length() - 1 - dg)
    return a


FIRE_G = pmul(FIRE_F1, FIRE_F2)


def fire_parity(m9):
    """bytes 0..1 for bytes 2..10: M(x) x^16 mod g(x)"""
    return pmod(int.from_bytes(bytes(m9), "big") << 16, FIRE_G)


def fire_syndrome(word11):
    """bytes 0..10 -> (remainder mod x^11+1, remainder mod x^5+...+1) of the systematic codeword M(x) x^16 + R(x)"""
    w = bytes(np.asarray(word11, np.uint8))
    c = (int.from_bytes(w[2:11], "big") << 16) | int.from_bytes(w[:2], "big")
    return pmod(c, FIRE_F1), pmod(c, FIRE_F2)


def fire_ok_model(superframes):
    """(n, >= 11) descrambled superframes -> n flags"""
    sf = np.asarray(superframes, np.uint8)
    return np.array([fire_syndrome(s[:11]) == (0, 0) for s in sf], np.uint8)


def with_fire_code(sf_bytes):
    """a superframe's bytes with bytes 0..1 set to the fire code of bytes 2..10"""
    sf = np.array(sf_bytes, np.uint8)
    r = fire_parity(sf[2:11])
    sf[0], sf[1] = r >> 8, r & 0xFF
    return sf


# ---- tests ----------------------------------------------------------------------------------------------------------

def test_prbs_first_bits_and_period():
    assert _PRBS[:16].tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 0]
    assert prbs_bytes_model(16).tolist() == [0x07, 0xBE]
    # maximal length: period 511 and no shorter one (511 = 7 * 73)
    assert np.array_equal(_PRBS[511:2 * 511], _PRBS[:511])
    for d in (7, 73):
        assert not np.array_equal(_PRBS[d:d + 511], _PRBS[:511])
    assert int(_PRBS[:511].sum()) == 256  # an m-sequence has 2^(n-1) ones per period


def test_scramble_is_self_inverse_and_keeps_padding():
    rng = np.random.default_rng(1)
    fr = rng.integers(0, 256, (5, 97), dtype=np.uint8)  # 770 bits: 2 padding bits in the last byte
    s = scramble(fr, 770)
    assert np.array_equal(scramble(s, 770), fr)
    assert np.array_equal(s[:, -1] & 0x3F, fr[:, -1] & 0x3F)


def test_crc16_genibus_check_value():
    assert crc16_genibus(b"123456789") == 0xD64E


def test_fib_crc_and_every_single_bit_flip():
    rng = np.random.default_rng(2)
    for _ in range(4):
        fib = make_fib(rng.integers(0, 256, 30, dtype=np.uint8))
        assert fib_ok_model(fib[None])[0] == 1
        bits = np.unpackbits(fib)
        flips = np.repeat(bits[None], 256, axis=0)
        flips[np.arange(256), np.arange(256)] ^= 1
        assert not fib_ok_model(np.packbits(flips, axis=1)).any()


def test_fire_code_generator():
    assert FIRE_G == (1 << 16) | 0x782F
    assert FIRE_G == sum(1 << k for k in (16, 14, 13, 12, 11, 5, 3, 2, 1, 0))


def test_fire_code_word_and_bursts():
    """a built word has syndrome 0; every burst of 1...11 bits anywhere in bytes 0..10 (the transmitted order, parity
    first) is detected"""
    rng = np.random.default_rng(3)
    for _ in range(3):
        w = with_fire_code(rng.integers(0, 256, 11, dtype=np.uint8))
        assert fire_syndrome(w) == (0, 0)
        bits = np.unpackbits(w)
        missed = 0
        for length in range(1, 12):
            inner = 1 << max(length - 2, 0)
            for start in range(0, 88 - length + 1):
                for pat in range(inner):
                    e = np.zeros(88, np.uint8)
                    e[start] = e[start + length - 1] = 1
                    for k in range(length - 2):
                        e[start + 1 + k] = (pat >> k) & 1
                    if fire_syndrome(np.packbits(bits ^ e)) == (0, 0):
                        missed += 1
        assert missed == 0


def test_library_prbs_matches_the_model(V):
    for fb in range(2, MAX_FRAMEBITS + 1, 2):
        got = V.prbs_bytes(fb)
        assert np.array_equal(got, prbs_bytes_model(fb)), fb
    assert V.prbs_bytes(0).size == 0
    buf = np.zeros(1160, np.uint8)
    for fb in (1, 3, 767, 9215, 9217, 9218, 0xFFFFFFFF):
        assert V.lib().vit_energy_dispersal_prbs(buf.ctypes.data_as(C.c_void_p), fb) == -1, fb
        with pytest.raises(ValueError):
            V.prbs_bytes(fb)
    assert V.lib().vit_energy_dispersal_prbs(None, 768) == -1
    assert not buf.any()


NEW_EXPORTS = ("vit_energy_dispersal_prbs", "vit_energy_dispersal_dev", "vit_energy_dispersal_varlen_dev",
               "vit_fib_crc_dev", "vit_decode_fic_dev", "vit_dabplus_punctured_superframes_dev")


def test_dab_exports(V):
    out = subprocess.check_output(["nm", "-D", "--defined-only", V.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in NEW_EXPORTS:
        assert name in exported and name in V.EXPORTS


def test_dab_calls_fail_loudly(V):
    """without a device: VIT_ERR_NO_DEVICE; with one, null buffers are VIT_ERR_ARG - nothing is launched either way"""
    import torch
    want = 1 if torch.cuda.is_available() else 2  # VIT_ERR_ARG / VIT_ERR_NO_DEVICE
    L = V.lib()
    assert L.vit_energy_dispersal_dev(None, 768, 4, None) == want
    assert L.vit_energy_dispersal_varlen_dev(None, 0, None, 4, None) == want
    assert L.vit_fib_crc_dev(None, 4, None, None) == want
    assert L.vit_decode_fic_dev(None, None, None, 768, 4, None, 128, None) == want
    assert L.vit_dabplus_punctured_superframes_dev(None, None, 128, None, None, None, None, 24, 4, None) == want
    if want == 2:
        assert "gfx950" in V.last_error()
