"""CPU-only: "From the FFT" (include/viterbi_amd.h) - the frequency interleaving table against its KATs, and the
demapper's definition as a numpy float32 model independent of the library, pinned by its properties and by a whole FIC
chain on the CPU (FIBs -> scramble -> encode -> puncture -> model transmitter -> model demapper -> depuncture -> oracle
decoder -> descramble -> FIB CRC).  tests/test_gpu_ofdm.py uses the same model as its byte-exact reference."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from test_dab_host import fib_ok_model, make_fib, scramble
from test_punct_host import depuncture, fic_segments, puncture

F32 = np.float32
MODE_I, MODE_II, MODE_III, MODE_IV = (2048, 1536, 76, 3, 4), (512, 384, 76, 3, 1), (256, 192, 153, 8, 1), (1024, 768, 76, 3, 2)
MODES = (MODE_I, MODE_II, MODE_III, MODE_IV)


# ---- the definition -------------------------------------------------------------------------------------------------

def freq_bins_model(nfft):
    """EN 300 401 clause 14.6: P(0) = 0, P(i) = (13 P(i-1) + nfft/4 - 1) mod nfft; the values in [nfft/8, 7 nfft/8] except
    nfft/2, in order, are d_n; QPSK symbol n travels on carrier d_n - nfft/2 -> (carriers k, FFT bins k mod nfft)"""
    p, d = 0, []
    for _ in range(1, nfft):
        p = (13 * p + nfft // 4 - 1) % nfft
        if nfft // 8 <= p <= 7 * nfft // 8 and p != nfft // 2:
            d.append(p)
    k = np.array(d, np.int64) - nfft // 2
    return k, k % nfft


def demap_model(z, bins, shape, gain):
    """z: (nframes, nsyms, nfft) complex64 FFT outputs -> (nframes, nsyms-1, 2K) soft bytes; every operation one numpy
    float32 operation (IEEE binary32, round to nearest even), in the order of the header"""
    nfft, K, nsyms = shape[0], shape[1], shape[2]
    z = np.asarray(z, np.complex64).reshape(-1, nsyms, nfft)[:, :, np.asarray(bins, np.int64)]
    assert z.shape[2] == K
    ar, ai, br, bi = z.real[:, 1:], z.imag[:, 1:], z.real[:, :-1], z.imag[:, :-1]
    assert ar.dtype == F32
    with np.errstate(all="ignore"):
        re = ar * br + ai * bi
        im = ai * br - ar * bi
        nrm = np.abs(re) + np.abs(im)
        ok = (nrm >= F32(2.0 ** -64)) & (nrm <= np.finfo(F32).max)
        s = F32(gain) / np.where(ok, nrm, F32(1))
        assert re.dtype == F32 and nrm.dtype == F32 and s.dtype == F32
        q0 = np.clip(F32(128) - np.rint(re * s), 0, 255)
        q1 = np.clip(F32(128) - np.rint(im * s), 0, 255)
    out = np.concatenate([np.where(ok, q0, 128), np.where(ok, q1, 128)], axis=2)
    return out.astype(np.uint8)


def split_model(out, shape, fic=None, ring=None, first_row=0, col=0):
    """where the model's bytes go: fic (nframes*fic_syms*2K bytes, flat) and ring (nrows, row_bytes) are updated in place"""
    nfft, K, nsyms, fic_syms, cifs = shape
    per = (nsyms - 1 - fic_syms) // cifs
    for t in range(out.shape[0]):
        for s in range(nsyms - 1):
            if s < fic_syms:
                if fic is not None:
                    fic[(t * fic_syms + s) * 2 * K:(t * fic_syms + s + 1) * 2 * K] = out[t, s]
            elif ring is not None:
                m = s - fic_syms
                row = (first_row + t * cifs + m // per) % ring.shape[0]
                ring[row, col + (m % per) * 2 * K:col + (m % per + 1) * 2 * K] = out[t, s]


def transmit(bits, bins, shape, rng, carrier_gain=None, snr_db=None, rotation=0.0):
    """the model transmitter and channel: bits (nframes, nsyms-1, 2K) of 0/1 -> (nframes, nsyms, nfft) complex64.
    QPSK symbol n of a data symbol = ((1 - 2 b[n]) + j (1 - 2 b[n+K])) / sqrt 2 on bin bins[n], differentially modulated
    (z_l = z_{l-1} q_l) from a reference symbol of random phases; carrier_gain (nfft complex) scales every symbol's
    bins, `rotation` turns everything by a common angle, AWGN at snr_db per carrier.  Unused bins are 0."""
    nfft, K, nsyms = shape[0], shape[1], shape[2]
    bits = np.asarray(bits, np.int64).reshape(-1, nsyms - 1, 2 * K)
    q = ((1 - 2 * bits[:, :, :K]) + 1j * (1 - 2 * bits[:, :, K:])) / np.sqrt(2.0)
    ref = np.exp(2j * np.pi * rng.random((bits.shape[0], 1, K)))
    car = np.concatenate([ref, q], axis=1).cumprod(axis=1)
    z = np.zeros((bits.shape[0], nsyms, nfft), np.complex128)
    z[:, :, np.asarray(bins, np.int64)] = car
    if carrier_gain is not None:
        z = z * np.asarray(carrier_gain)[None, None, :]
    z = z * np.exp(1j * rotation)
    if snr_db is not None:
        sigma = np.sqrt(10.0 ** (-snr_db / 10.0) / 2.0)
        noise = sigma * (rng.standard_normal(z.shape) + 1j * rng.standard_normal(z.shape))
        used = np.zeros(nfft, bool)
        used[np.asarray(bins, np.int64)] = True
        z = z + noise * used[None, None, :]
    return z.astype(np.complex64)


def random_carrier_gain(rng, nfft):
    """a frequency-selective channel: magnitudes 0.3 ... 3, any phase"""
    return rng.uniform(0.3, 3.0, nfft) * np.exp(2j * np.pi * rng.random(nfft))


# ---- frequency interleaving -----------------------------------------------------------------------------------------

KAT_FIRST = {2048: [-513, -14, 329, 692, -733, 13], 512: [-129, -14, -55], 256: [-65, -14, 52], 1024: [-257, -14, 73]}


def test_freq_interleave_bins_kats(V):
    for nfft, first in KAT_FIRST.items():
        bins = V.freq_interleave_bins(nfft)
        assert bins.dtype == np.uint16 and bins.size == 3 * nfft // 4
        assert len(set(bins.tolist())) == bins.size and 0 not in bins and bins.max() < nfft
        k = np.where(bins.astype(np.int64) >= nfft // 2, bins.astype(np.int64) - nfft, bins.astype(np.int64))
        assert k[:len(first)].tolist() == first
        assert np.abs(k).max() == 3 * nfft // 8 and np.abs(k).min() == 1  # carriers -K/2 ... K/2 without DC
        mk, mb = freq_bins_model(nfft)
        assert np.array_equal(k, mk) and np.array_equal(bins, mb)
    bins = V.freq_interleave_bins(2048)
    assert bins[:6].tolist() == [1535, 2034, 329, 692, 1315, 13]
    assert bins[-3:].tolist() == [652, 606, 197]


def test_freq_interleave_bins_rejects_other_lengths(V):
    buf = np.full(8192, 0xEEEE, np.uint16)
    for nfft in (0, 1, 64, 128, 255, 257, 4096, 8192, 2047, 0xFFFFFFFF):
        assert V.lib().vit_freq_interleave_bins(nfft, buf.ctypes.data_as(C.c_void_p)) == -1, nfft
        with pytest.raises(ValueError):
            V.freq_interleave_bins(nfft)
    assert V.lib().vit_freq_interleave_bins(2048, None) == -1
    assert (buf == 0xEEEE).all()


# ---- the model's properties -----------------------------------------------------------------------------------------

def small_case(rng, shape=MODE_III, nframes=2):
    nfft, K, nsyms = shape[0], shape[1], shape[2]
    bins = freq_bins_model(nfft)[1]
    bits = rng.integers(0, 2, (nframes, nsyms - 1, 2 * K))
    return bins, bits


def test_noise_free_bytes_and_decisions():
    rng = np.random.default_rng(1)
    bins, bits = small_case(rng)
    z = transmit(bits, bins, MODE_III, rng)
    for gain in (127.0, 180.0, 254.0, 2.0):
        out = demap_model(z, bins, MODE_III, gain)
        assert np.array_equal(out > 128, bits.astype(bool)), gain
        ideal = np.where(bits == 1, 128 + gain / 2, 128 - gain / 2)
        assert np.abs(out.astype(np.float64) - np.clip(ideal, 0, 255)).max() <= 1, gain


def test_rotation_and_carrier_gain_change_no_decision():
    rng = np.random.default_rng(2)
    bins, bits = small_case(rng, MODE_II, 1)
    state = rng.bit_generator.state
    base = demap_model(transmit(bits, bins, MODE_II, rng), bins, MODE_II, 200.0)
    rng.bit_generator.state = state  # the same reference phases
    turned = demap_model(transmit(bits, bins, MODE_II, rng, carrier_gain=random_carrier_gain(rng, 512), rotation=1.234),
                         bins, MODE_II, 200.0)
    assert np.array_equal(base > 128, bits.astype(bool)) and np.array_equal(turned > 128, bits.astype(bool))
    assert np.abs(base.astype(int) - turned.astype(int)).max() <= 1  # float rounding at most


def special_carriers(z, bins, sym):
    """overwrites carriers 0 ... 5 of symbol `sym` of every frame: zero, 2^-70 magnitude, NaN, Inf, mixed NaN, huge"""
    z[:, sym, bins[0]] = 0
    z[:, sym, bins[1]] = F32(2.0 ** -70) * (1 + 1j)
    z[:, sym, bins[2]] = np.nan
    z[:, sym, bins[3]] = np.inf
    z[:, sym, bins[4]] = complex(1.0, np.nan)
    z[:, sym, bins[5]] = complex(3e38, 3e38)  # the product overflows to Inf
    return 6


def test_special_carriers_are_erasures():
    rng = np.random.default_rng(3)
    bins, bits = small_case(rng)
    K = MODE_III[1]
    z = transmit(bits, bins, MODE_III, rng)
    n = special_carriers(z, bins, 5)
    out = demap_model(z, bins, MODE_III, 254.0)
    for s in (4, 5):  # symbol 5 is `a` of data symbol 4 and `b` of data symbol 5
        assert (out[:, s, :n] == 128).all() and (out[:, s, K:K + n] == 128).all()
    assert not (out[:, 3, :n] == 128).any() and np.array_equal(out[:, 6:] > 128, bits[:, 6:].astype(bool))
    # 2^-70 times a unit carrier: nrm ~ 2^-69.5 < 2^-64 although nothing is denormal yet
    assert np.abs(z[0, 5, bins[1]]) > 1e-22


def test_clamping_at_the_largest_gain():
    rng = np.random.default_rng(4)
    bins, bits = small_case(rng)
    out = demap_model(transmit(bits, bins, MODE_III, rng), bins, MODE_III, 65536.0)
    assert np.array_equal(out, np.where(bits == 1, 255, 0))


def test_ties_round_to_even():
    """re*s exactly k + 0.5 from small integers: b = 1 and a = x + jy with x + y = 8 give y = a, nrm = 8 and at gain 4
    s = 1/2 exactly, so re*s = x/2 is a tie for odd x"""
    K = 4
    shape = (64, K, 2, 1, 1)
    bins = np.array([1, 2, 3, 4])
    z = np.zeros((1, 2, 64), np.complex64)
    z[0, 0, bins] = 1.0
    # y = a: re + im = 8 -> s = gain/8 exactly; gain 4: re*s = re/2, a tie for odd re
    z[0, 1, bins] = [complex(1, 7), complex(3, 5), complex(5, 3), complex(7, 1)]
    out = demap_model(z, bins, shape, 4.0)[0, 0]
    # rint(0.5) = 0, rint(1.5) = 2, rint(2.5) = 2, rint(3.5) = 4
    assert out[:K].tolist() == [128, 126, 126, 124] and out[K:].tolist() == [124, 126, 126, 128]


# ---- the chain on the CPU -------------------------------------------------------------------------------------------

def fic_bits(O, rng, nframes):
    """nframes mode-I frames' FIC: 4 coding blocks of 3 FIBs each -> (payload FIBs (nframes*4, 96 bytes), transmitted bits
    (nframes, 3, 3072))"""
    nblk = 4 * nframes
    fibs = np.stack([np.concatenate([make_fib(rng.integers(0, 256, 30, dtype=np.uint8)) for _ in range(3)])
                     for _ in range(nblk)])
    coded = np.stack([O.encode(b) for b in np.unpackbits(scramble(fibs, 768), axis=1)])
    tx = puncture(coded.astype(np.uint8), fic_segments(), 768)
    assert tx.shape == (nblk, 2304) and tx.max() == 1
    return fibs, tx.reshape(nframes, 3, 3072)


def fic_decode(O, soft):
    """soft bytes of FIC blocks (n, 2304) -> descrambled FIBs (n, 96)"""
    return scramble(O.decode_batch(768, depuncture(soft, fic_segments(), 768, 128), nthreads=8), 768)


@pytest.mark.parametrize("gain", [127.0, 180.0, 254.0])
def test_fic_chain_on_the_cpu(O, gain):
    """mode I, 8 frames (96 FIBs), a random per-carrier gain and AWGN at 11 dB carrier SNR: every FIB CRC holds and the
    FIBs are the ones sent"""
    rng = np.random.default_rng(20)
    nframes = 8
    bins = freq_bins_model(2048)[1]
    fibs, tx = fic_bits(O, rng, nframes)
    bits = rng.integers(0, 2, (nframes, 75, 3072))
    bits[:, :3] = tx
    z = transmit(bits, bins, MODE_I, rng, carrier_gain=random_carrier_gain(rng, 2048), snr_db=11.0)
    out = demap_model(z, bins, MODE_I, gain)
    got = fic_decode(O, out[:, :3].reshape(-1, 2304))
    assert fib_ok_model(got.reshape(-1, 32)).all()
    assert np.array_equal(got, fibs)


# ---- the library without a GPU --------------------------------------------------------------------------------------

NEW_EXPORTS = ("vit_freq_interleave_bins", "vit_ofdm_demap_dev")


def test_ofdm_exports(V):
    out = subprocess.check_output(["nm", "-D", "--defined-only", V.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in NEW_EXPORTS:
        assert name in exported and name in V.EXPORTS


def test_ofdm_call_fails_loudly(V):
    """without a device: VIT_ERR_NO_DEVICE and an error text naming gfx950; with one, NULL buffers are VIT_ERR_ARG -
    nothing is launched either way; the host helper works without one"""
    import torch
    want = 1 if torch.cuda.is_available() else 2  # VIT_ERR_ARG / VIT_ERR_NO_DEVICE
    shape = V.OfdmShape(*MODE_I)
    assert V.lib().vit_ofdm_demap_dev(None, 2048, 76 * 2048, None, C.byref(shape), 254.0, 1, None, None, 0, None) == want
    if want == 2:
        assert "gfx950" in V.last_error()
    assert C.sizeof(V.OfdmShape) == 20 and V.OfdmShape.cifs.offset == 16
    assert V.OFDM_MODES == {1: MODE_I, 2: MODE_II, 3: MODE_III, 4: MODE_IV}
    assert V.freq_interleave_bins(256).size == 192
