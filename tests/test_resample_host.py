"""CPU-only: "Before the stream: rate conversion and channel selection" (include/viterbi_amd.h) - the definition of
vit_iq_resample_dev as a numpy float32 model independent of the library (resample_model: one float32 ufunc per operation,
an output's terms in four accumulators, term k in accumulator k mod 4), the two host helpers vit_resample_taps and
vit_resample_out_count against their formulas, the model's properties (continuation, independence of nchan, the pure
delay), and a whole chain without noise: a mode-I frame sequence synthesised at 2.5 MS/s with a 200 kHz offset, resampled
by the model and fed through acquire_model, sync_model, the demodulator's model and the oracle's FIC decoder.
tests/test_gpu_resample.py uses resample_model as its exact reference and replays argument_error_cases()."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from test_acq_host import Acq, acquire_model
from test_dab_host import fib_ok_model
from test_fft_host import F32, cmul_model, front_model, nco_model, twiddles_model, useful_parts
from test_ofdm_host import MODE_I, demap_model, fic_bits, fic_decode, freq_bins_model
from test_sync_host import Params, prs_table, sync_model

MAX_CHAN = 16
_nco = {}  # nco_model(bits), built once


class Rs:
    """vit_resample_params: taps float32 (L, T); rot None or (nchan, 2) of {phase0, step}"""

    def __init__(self, L, M, taps, pos0=0, rot=None, nco_bits=0):
        self.L, self.M, self.taps, self.pos0, self.nco_bits = L, M, np.ascontiguousarray(taps, F32), pos0, nco_bits
        assert self.taps.shape[0] == L
        self.T = self.taps.shape[1]
        self.rot = None if rot is None else np.asarray(rot, np.int64).reshape(-1, 2) % (1 << 32)
        self.nchan = 1 if rot is None else self.rot.shape[0]

    def alone(self, c):
        """channel c in a call of its own"""
        return Rs(self.L, self.M, self.taps, self.pos0, self.rot[c:c + 1], self.nco_bits)


# ---- the definition -------------------------------------------------------------------------------------------------

def out_count_model(nsamples, L, M, T, pos0=0):
    """the largest nout whose last output has n0 + T <= nsamples (and P < 2^64), clamped to 2^63 - 1"""
    if nsamples < T:
        return 0
    pmax = min((nsamples - T + 1) * L - 1, (1 << 64) - 1)
    return 0 if pos0 > pmax else min((pmax - pos0) // M + 1, (1 << 63) - 1)


def taps_formula(L, T, cutoff):
    """the Blackman-windowed sinc of the header in binary64 -> float64 (L, T), every phase divided by its sum"""
    u = np.arange(T, dtype=np.float64)[None, :] - (T // 2 - 1) - np.arange(L, dtype=np.float64)[:, None] / L
    h = 2.0 * cutoff * np.sinc(2.0 * cutoff * u) * (0.42 + 0.5 * np.cos(2.0 * np.pi * u / T) + 0.08 * np.cos(4.0 * np.pi * u / T))
    return h / h.sum(axis=1, keepdims=True)


def rotated_model(x, r, c, n_first=0):
    """step B for channel c: x complex64, sample i is sample n_first + i of d_iq -> (re, im) float32"""
    x = np.asarray(x, np.complex64)
    re, im = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
    if r.rot is None:
        return re, im
    if r.nco_bits not in _nco:
        _nco[r.nco_bits] = nco_model(r.nco_bits)
    nco = _nco[r.nco_bits]
    n = (np.uint64(n_first) + np.arange(x.size, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)
    ph = (np.uint64(r.rot[c, 0]) + n * np.uint64(r.rot[c, 1])) & np.uint64(0xFFFFFFFF)  # < 2^64: both factors < 2^32
    w = nco[(ph >> np.uint64(32 - r.nco_bits)).astype(np.int64)]
    with np.errstate(all="ignore"):
        return cmul_model(re, im, np.ascontiguousarray(w[:, 0]), np.ascontiguousarray(w[:, 1]))


def resample_model(floats, r, nout):
    """floats: the samples x[n] (complex64, 1-D; only those an output needs are touched); r: Rs -> complex64 (nchan, nout)"""
    x = np.asarray(floats, np.complex64)
    wide = r.pos0 + nout * r.M >= 1 << 62  # P as Python integers where int64 would not hold it
    P = r.pos0 + np.arange(nout, dtype=object if wide else np.int64) * r.M
    n0, phi = np.asarray(P // r.L, np.int64), np.asarray(P % r.L, np.int64)
    assert nout == 0 or int(n0[-1]) + r.T <= x.size
    out = np.zeros((r.nchan, nout), np.complex64)
    if nout == 0:
        return out
    lo, hi = int(n0[0]), int(n0[-1]) + r.T
    for c in range(r.nchan):
        y = rotated_model(x[lo:hi], r, c, n_first=lo)
        for comp, part in enumerate(y):
            acc = [np.zeros(nout, F32) for _ in range(4)]
            with np.errstate(all="ignore"):
                for k in range(r.T):
                    term = r.taps[phi, k] * part[n0 - lo + k]
                    assert term.dtype == F32
                    acc[k % 4] = acc[k % 4] + term
                res = (acc[0] + acc[1]) + (acc[2] + acc[3])
            assert res.dtype == F32
            if comp == 0:
                out[c].real = res
            else:
                out[c].imag = res
    return out + np.complex64(0)  # by value: -0 = +0


def random_taps(rng, L, T):
    """taps of any shape for the tests of the arithmetic: |g| <= 1, exact zeros among them"""
    g = rng.uniform(-1.0, 1.0, (L, T)).astype(F32)
    g[rng.random((L, T)) < 0.05] = 0.0
    return g


# ---- the host helpers -------------------------------------------------------------------------------------------------

def ulps_apart(a, b):
    a, b = np.asarray(a, F32).view(np.int32).astype(np.int64), np.asarray(b, F32).view(np.int32).astype(np.int64)
    a, b = np.where(a < 0, -(a & 0x7FFFFFFF), a), np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


@pytest.mark.parametrize("L,T,cutoff", [(1, 4, 0.5), (1, 8, 0.25), (3, 4, 0.1), (128, 16, 0.45), (512, 32, 0.4096),
                                        (128, 128, 0.1024), (1024, 16, 0.3), (7, 128, 0.5)])
def test_taps_builder(V, L, T, cutoff):
    got = V.resample_taps(L, T, cutoff)
    want = taps_formula(L, T, cutoff)
    assert got.shape == (L, T) and got.dtype == F32
    # libm and numpy may differ in the last binary64 bit, which moves a rounding to binary32 by at most one unit
    assert ulps_apart(got, want.astype(F32)).max() <= 1
    assert np.abs(got.astype(np.float64).sum(axis=1) - 1.0).max() <= 2.0 ** -22
    # the peak of phase 0 sits at tap T/2 - 1: the delay the header names
    assert int(np.argmax(got[0])) == T // 2 - 1


def test_taps_builder_rejections(V):
    buf = np.full(16384 + 8, 7.0, F32)
    p = buf.ctypes.data_as(C.c_void_p)
    f = V.lib().vit_resample_taps
    for L, T, cutoff in ((0, 4, 0.25), (1025, 4, 0.25), (1, 0, 0.25), (1, 2, 0.25), (1, 6, 0.25), (1, 132, 0.25), (1024, 32, 0.25),
                         (129, 128, 0.25), (4, 8, 0.0), (4, 8, -0.1), (4, 8, 0.5000001), (4, 8, float("nan")),
                         (4, 8, float("inf"))):
        assert f(L, T, cutoff, p) == -1, (L, T, cutoff)
        assert "bad arguments" in V.last_error()
    assert f(4, 8, 0.25, None) == -1
    assert (buf == 7.0).all()
    assert f(128, 128, 0.5, p) == 16384 and f(1024, 16, 0.01, p) == 16384 and (buf[16384:] == 7.0).all()
    with pytest.raises(ValueError):
        V.resample_taps(4, 6, 0.25)
    with pytest.raises(ValueError):
        V.resample_taps(4, 8, 0.75)


def test_out_count(V):
    """against a brute-force count over a grid, nsamples < T among it, and at the edges of the 64-bit arithmetic"""
    def brute(ns, L, M, T, pos0):
        m = 0
        while (pos0 + m * M) // L + T <= ns:
            m += 1
        return m

    n = 0
    for L, M, T in ((1, 1, 4), (1, 2, 8), (3, 7, 4), (128, 125, 16), (512, 625, 32), (2, 4096, 4), (1024, 1, 4)):
        for ns in (0, 1, T - 1, T, T + 1, 2 * T + 3, 97, 400):
            for pos0 in (0, 1, L - 1, L, 5 * L + 2, 90 * L, 396 * L + L - 1, 1000 * L):
                want = brute(ns, L, M, T, pos0)
                assert out_count_model(ns, L, M, T, pos0) == want
                assert V.resample_out_count(ns, L, M, T, pos0) == want, (ns, L, M, T, pos0)
                n += 1
    assert n > 400
    big = (1 << 60) - 1
    for ns, L, M, T, pos0 in ((big, 1, 1, 4, 0), (big, 1024, 1, 4, 0), (big, 1024, 4096, 4, (1 << 64) - 1), (big, 1, 4096, 128, 12345),
                              (1 << 40, 512, 625, 32, 1 << 45)):
        assert V.resample_out_count(ns, L, M, T, pos0) == out_count_model(ns, L, M, T, pos0)
    f = V.lib().vit_resample_out_count
    assert f(100, None) == -1
    for L, M, T in ((0, 1, 4), (1025, 1, 4), (1, 0, 4), (1, 4097, 4), (1, 1, 0), (1, 1, 6), (1, 1, 132), (1024, 1, 32)):
        par = V.ResampleParams(L, M, T, 1, 0, None, None, 0, 0, None)
        assert f(100, C.byref(par)) == -1, (L, M, T)
        with pytest.raises(ValueError):
            V.resample_out_count(100, L, M, T)


# ---- the model's properties ---------------------------------------------------------------------------------------------

def noise(rng, n):
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5)).astype(np.complex64)


ROT5 = [(0, 0), (12345, 0x10000000), (0xFFFFFFF0, 0xF0000001), (7, 3), (0x80000000, 0x7FFFFFFF)]


def continuation(r, m1):
    """the stream-continuation rule of the header after m1 outputs -> (s: samples dropped, the second call's Rs)"""
    P = r.pos0 + m1 * r.M
    s = P // r.L
    rot = None if r.rot is None else np.stack([(r.rot[:, 0] + s * r.rot[:, 1]) % (1 << 32), r.rot[:, 1]], axis=1)
    return s, Rs(r.L, r.M, r.taps, P - s * r.L, rot, r.nco_bits)


@pytest.mark.parametrize("L,M,T", [(3, 7, 4), (128, 125, 16), (512, 625, 32), (5, 2, 8)])
def test_continuation_in_every_bit(L, M, T):
    """one stream split at three points: the pieces equal the long call, with rotation on"""
    rng = np.random.default_rng(L + M)
    x = noise(rng, 3000)
    r = Rs(L, M, random_taps(rng, L, T), pos0=2 * L + L // 2, rot=ROT5[1:4], nco_bits=12)
    nout = out_count_model(x.size, L, M, T, r.pos0)
    whole = resample_model(x, r, nout)
    cuts = [0, nout // 7, nout // 2 + 1, nout - 3, nout]
    skipped, cur = 0, r
    for a, b in zip(cuts[:-1], cuts[1:]):
        part = resample_model(x[skipped:], cur, b - a)
        assert np.array_equal(part.view(np.uint32), whole[:, a:b].view(np.uint32)), (a, b)
        s, cur = continuation(cur, b - a)
        assert 0 <= cur.pos0 < L
        skipped += s
    assert skipped > 0


def test_a_channel_alone_equals_that_channel_among_five():
    rng = np.random.default_rng(5)
    x = noise(rng, 2000)
    r = Rs(128, 625, random_taps(rng, 128, 16), pos0=77, rot=ROT5, nco_bits=10)
    nout = out_count_model(x.size, r.L, r.M, r.T, r.pos0)
    five = resample_model(x, r, nout)
    for c in range(5):
        assert np.array_equal(resample_model(x, r.alone(c), nout)[0].view(np.uint32), five[c].view(np.uint32))
    assert not np.array_equal(five[1], five[2])
    # a step of 0 with phase0 = 0 multiplies by the exact 1: the input's filter without rotation
    plain = resample_model(x, Rs(r.L, r.M, r.taps, r.pos0), nout)
    assert np.array_equal(plain[0], five[0])


def test_pure_delay_and_the_four_accumulators():
    """L = M = 1, T = 4, taps {0, 1, 0, 0}: the input delayed by one sample, by value; and the grouping of the sum, on values
    where a serial sum or a tree of adjacent pairs gives another result"""
    rng = np.random.default_rng(6)
    x = noise(rng, 100)
    out = resample_model(x, Rs(1, 1, [[0, 1, 0, 0]]), 97)
    assert np.array_equal(out[0], x[1:98])
    # T = 8, all taps 1: accumulators {x0 + x4, x1 + x5, x2 + x6, x3 + x7}, then (a0 + a1) + (a2 + a3)
    v = np.array([2.0 ** 24, 1, 1, 1, 1, 1, 1, 1], F32)
    got = resample_model(v.astype(np.complex64), Rs(1, 1, np.ones((1, 8), F32)), 1)[0, 0].real
    # a0 = 2^24 + 1 -> 2^24 (the one is lost), a1 = a2 = a3 = 2: (2^24 + 2) + 4
    assert got == F32(2.0 ** 24 + 6)
    serial = F32(0)
    for t in v:
        serial = F32(serial + t)
    assert serial == F32(2.0 ** 24) and got != serial
    # phases: L = 2, M = 3 walks n0 = 0, 1, 3, 4, ... and phi = 0, 1, 0, 1
    taps = np.array([[1, 0, 0, 0], [0, 0, 1, 0]], F32)
    ramp = np.arange(40).astype(np.complex64)
    assert resample_model(ramp, Rs(2, 3, taps), 6)[0].real.tolist() == [0, 1 + 2, 3, 4 + 2, 6, 7 + 2]
    assert resample_model(ramp, Rs(2, 3, taps, pos0=5), 3)[0].real.tolist() == [2 + 2, 4, 5 + 2]


def test_reads_only_what_the_outputs_need():
    """NaN in front of the first needed sample, behind the last one and - with M > L*T - in the gaps: no output is touched"""
    rng = np.random.default_rng(7)
    x = noise(rng, 400)
    r = Rs(3, 7, random_taps(rng, 3, 4), pos0=5 * 3 + 2)
    nout = 20
    want = resample_model(x, r, nout)
    y = x.copy()
    y[:5] = np.nan
    y[(r.pos0 + (nout - 1) * r.M) // r.L + r.T:] = np.nan
    assert np.array_equal(resample_model(y, r, nout), want)
    g = Rs(1, 9, random_taps(rng, 1, 4))
    y = x.copy()
    for m in range(40):
        y[9 * m + 4:9 * m + 9] = np.nan
    assert not np.isnan(resample_model(y, g, 40)).any()


# ---- the whole chain, noise-free ---------------------------------------------------------------------------------------

FS_IN, FS_OUT, OFFSET_HZ = 2.5e6, 2.048e6, 200.0e3
CHAIN_FRAMES = 3
CHAIN_CUTOFF = 1.024e6 / FS_IN  # between the passband's end, 768 kHz, and the stopband's start, 1.28 MHz
_chain = {}


def chain_case(O):
    """CHAIN_FRAMES mode-I transmission frames (null symbol of 2656 sample periods of 2.048 MS/s, then 76 symbols of 2552)
    sampled at 2.5 MS/s on a carrier 200 kHz off: sample j lies at t = j * 2048/2500 periods, and a symbol's OFDM sum
    sum_k z[k] exp(2 pi i k (t - u) / 2048), u the start of its useful part, is there sum_k (z[k] exp(-2 pi i k u / 2048))
    exp(2 pi i k j / 2500): an inverse DFT of length 2500, in binary64.  -> (x complex64, fibs sent, prs, bins), built once"""
    if not _chain:
        rng = np.random.default_rng(2500)
        nfft, K, nsyms = MODE_I[:3]
        bins = freq_bins_model(nfft)[1]
        k = np.where(bins >= nfft // 2, bins - nfft, bins).astype(np.int64)  # carrier numbers
        prs = prs_table(rng, nfft, bins)
        fibs, tx = fic_bits(O, rng, CHAIN_FRAMES)
        bits = rng.integers(0, 2, (CHAIN_FRAMES, nsyms - 1, 2 * K))
        bits[:, :3] = tx
        q = ((1 - 2 * bits[:, :, :K]) + 1j * (1 - 2 * bits[:, :, K:])) / np.sqrt(2.0)
        ref = np.broadcast_to(np.asarray(prs, np.complex128)[bins], (CHAIN_FRAMES, 1, K))
        car = np.concatenate([ref, q], axis=1).cumprod(axis=1)  # (frames, nsyms, K)
        null, S, G = 2656, 2552, 504
        frame = null + nsyms * S
        lead = 700  # periods of silence in front of the first null
        total = lead + CHAIN_FRAMES * frame + null
        nin = int(total * 2500 // 2048)
        x = np.zeros(nin, np.complex128)
        for f in range(CHAIN_FRAMES):
            for l in range(nsyms):
                t0 = lead + f * frame + null + l * S  # the symbol's guard starts here, its useful part at u
                u = t0 + G
                j0, j1 = -(-t0 * 2500 // 2048), -(-(t0 + S) * 2500 // 2048)  # samples with t0 <= t < t0 + S
                z = np.zeros(2500, np.complex128)
                z[k % 2500] = car[f, l] * np.exp(-2j * np.pi * k * u / 2048.0)
                period = np.fft.ifft(z) * 2500
                x[j0:j1] = period[np.arange(j0, j1) % 2500]
        x *= np.exp(2j * np.pi * (OFFSET_HZ / FS_IN) * np.arange(nin))
        _chain["case"] = ((x / nfft).astype(np.complex64), fibs, prs, bins)
    return _chain["case"]


def chain_params(V=None):
    """-> (Rs of the 2.5 MS/s channel, Acq, Params): 512/625 with 32 taps, the offset taken away by the rotation"""
    taps = taps_formula(512, 32, CHAIN_CUTOFF).astype(F32) if V is None else V.resample_taps(512, 32, CHAIN_CUTOFF)
    step = int(round(-OFFSET_HZ / FS_IN * 2.0 ** 32)) % (1 << 32)
    r = Rs(512, 625, taps, rot=[(0, step)], nco_bits=12)
    # the edge is the first guard's start, found up to a block and half the filter's length (45 periods) early: the coarse
    # start is the first useful sample give or take 23
    a = Acq(32, 64, 32, 6144, offset=504 + 22)
    prm = Params(2048, 504, 76, 64, 2, cp_symbols=4, backoff=252)
    return r, a, prm


def fic_of(x, starts, rots, prm, bins):
    """the demodulator's model on the frames at `starts` -> FIC soft bytes (nframes*4, 2304)"""
    tw, nco = twiddles_model(prm.nfft), nco_model(12)
    soft = []
    for s, rot in zip(starts, rots):
        parts = useful_parts(x, int(s), (prm.nfft, 0, 4), prm.sym_stride)[None]
        z = front_model(parts, tw, nco, 12, [rot], prm.sym_stride)
        soft.append(demap_model(z, bins, (prm.nfft, len(bins), 4), 254.0)[0])
    return np.stack(soft).reshape(-1, 2304)


def test_whole_chain_without_noise(O):
    """wideband capture -> resample -> acquire -> sync -> demod -> FIC decode: every FIB CRC holds and the FIBs are those sent"""
    x, fibs, prs, bins = chain_case(O)
    r, a, prm = chain_params()
    nout = out_count_model(x.size, r.L, r.M, r.T)
    y = resample_model(x, r, nout)[0]
    coarse, info, _ = acquire_model(y, a, CHAIN_FRAMES)
    # the first guard starts 700 + 2656 periods behind sample 0; output m sits at input time m*M/L + T/2 - 1, so in y
    # everything lies 15 input samples = 12.3 periods earlier
    edge = 700 + 2656 - 15 * 2048.0 / 2500.0
    print("coarse", coarse.tolist(), "edges", [edge + f * 196608 for f in range(CHAIN_FRAMES)], "q", info[:, 1].view(F32).tolist())
    assert (coarse != -1).all()
    # the filter reaches T/2 input samples ahead, so the power comes back that much in front of the edge, and the search
    # names the start of the block that holds it
    err = coarse - a.offset - (edge + 196608 * np.arange(CHAIN_FRAMES))
    assert (err <= 0).all() and (err > -(a.B + (r.T // 2) * r.L / r.M)).all(), err
    start, rot, sinfo, _ = sync_model(y, coarse, prm, prs, twiddles_model(2048), nco_model(12), 12)
    print("start", start.tolist(), "mhat/tau", sinfo[:, :2].view(np.int32).tolist())
    assert (start != -1).all() and (sinfo[:, 0] == 0).all()  # no carrier offset is left
    # the fine start sits in the guard: the true useful start is edge + 504, backoff 252
    assert (np.abs(start + prm.backoff - (edge + 504 + 196608 * np.arange(CHAIN_FRAMES))) <= 2).all()
    got = fic_decode(O, fic_of(y, start, rot, prm, bins))
    assert fib_ok_model(got.reshape(-1, 32)).all()
    assert np.array_equal(got, fibs)
    # without the rotation the ensemble lies 200 carriers off: the resampler's filter cuts into it and nothing decodes
    plain = resample_model(x, Rs(r.L, r.M, r.taps), nout)[0]
    bad = fic_decode(O, fic_of(plain, start, rot, prm, bins))
    assert not fib_ok_model(bad.reshape(-1, 32)).any()


# ---- the library without a GPU --------------------------------------------------------------------------------------

NEW_EXPORTS = ("vit_resample_taps", "vit_resample_out_count", "vit_iq_resample_dev")


def test_resample_exports(V):
    out = subprocess.check_output(["nm", "-D", "--defined-only", V.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in NEW_EXPORTS:
        assert name in exported and name in V.EXPORTS
    P = V.ResampleParams
    assert C.sizeof(P) == 56 and [getattr(P, f).offset for f, _ in P._fields_] == [0, 4, 8, 12, 16, 24, 32, 40, 44, 48]
    assert V.RESAMPLE_MAX_CHAN == MAX_CHAN and callable(V.iq_resample_dev)
    # the tile rule the GPU tests place their sizes around
    assert V.resample_tile(1, 1, 4) == (1024, False) and V.resample_tile(512, 625, 32) == (1024, False)
    assert V.resample_tile(128, 625, 128) == (256, False) and V.resample_tile(1024, 4096, 4) == (512, False)
    assert V.resample_tile(1, 128, 128) == (16, False) and V.resample_tile(1, 9, 4) == (512, True)  # a span of 2048; gaps


def argument_error_cases():
    """every rule of vit_iq_resample_dev that is VIT_ERR_ARG -> a list of (description, kwargs) for `resample_call` below:
    the base call is float32, L/M = 3/7 with T = 8, 2 channels, 4096 samples, nout 100 at out_stride 128"""
    nan, inf = float("nan"), float("inf")
    cases = [("NULL d_iq", dict(iq=None)), ("NULL p", dict(null_p=True)), ("NULL d_taps", dict(taps=None)),
             ("NULL d_out", dict(out=None)), ("nout < 0", dict(nout=-1)),
             ("float32 d_iq at 4 bytes", dict(iq_off=4)), ("cu8 d_iq at 2 bytes", dict(iq_off=2, fmt=(1, 1.0))),
             ("cs16 d_iq at 2 bytes", dict(iq_off=2, fmt=(3, 1.0))), ("d_taps at 4 bytes", dict(taps_off=4)),
             ("d_nco at 4 bytes", dict(nco_off=4)), ("d_out at 4 bytes", dict(out_off=4)),
             ("L = 0", dict(par=dict(L=0))), ("L = 1025", dict(par=dict(L=1025))), ("M = 0", dict(par=dict(M=0))),
             ("M = 4097", dict(par=dict(M=4097))), ("T = 0", dict(par=dict(T=0))), ("T = 6", dict(par=dict(T=6))),
             ("T = 132", dict(par=dict(T=132))), ("L*T = 16416", dict(par=dict(L=513, T=32))),
             ("nchan = 0", dict(par=dict(nchan=0))), ("nchan = 17", dict(par=dict(nchan=17))),
             ("nco_bits = 0", dict(par=dict(nco_bits=0))), ("nco_bits = 21", dict(par=dict(nco_bits=21))),
             ("reserved = 1", dict(par=dict(reserved=1))), ("rot without d_nco", dict(nco=None)),
             ("d_nco without rot", dict(rot=None, par=dict(nchan=1))), ("no rot, nchan 2", dict(rot=None, nco=None)),
             ("unknown format", dict(fmt=(4, 1.0))), ("cu8 scale 0", dict(fmt=(1, 0.0))), ("cs8 scale NaN", dict(fmt=(2, nan))),
             ("cs16 scale 2^17", dict(fmt=(3, 2.0 ** 17))), ("cs16 scale Inf", dict(fmt=(3, inf))),
             ("nsamples = 2^60", dict(nsamples=1 << 60)), ("nout one more than the stream holds", dict(nout="count+1", nsamples=240)),
             ("pos0 beyond the stream", dict(par=dict(pos0=3 * 4096), nout=1)),
             ("nsamples < T", dict(nsamples=7, nout=1)), ("out_stride < nout with 2 channels", dict(out_stride=99))]
    return cases


def resample_call(V, torch, bufs, iq="buf", iq_off=0, nsamples=4096, fmt=None, par=None, null_p=False, taps="buf", taps_off=0,
                  nco="buf", nco_off=0, rot="buf", out="buf", out_off=0, nout=100, out_stride=128):
    """one raw call of the C ABI on the buffers of resample_buffers -> its return value"""
    P = lambda t, off: None if t is None else C.c_void_p(t.data_ptr() + off)  # noqa: E731
    p = dict(L=3, M=7, T=8, nchan=2, pos0=0, nco_bits=8, reserved=0)
    p.update(par or {})
    pairs = (C.c_uint32 * (2 * MAX_CHAN))(*([5, 0x01000000] * MAX_CHAN))
    rp = V.ResampleParams(p["L"], p["M"], p["T"], p["nchan"], p["pos0"], P(bufs["taps"] if taps == "buf" else None, taps_off),
                          P(bufs["nco"] if nco == "buf" else None, nco_off), p["nco_bits"], p["reserved"],
                          C.cast(pairs, C.c_void_p) if rot == "buf" else None)
    if nout in ("count", "count+1"):
        nout = V.lib().vit_resample_out_count(nsamples, C.byref(rp)) + (nout == "count+1")
        assert 100 <= nout <= 101
    f = None if fmt is None else C.byref(V.IqFormat(*fmt))
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return V.lib().vit_iq_resample_dev(P(bufs["iq"] if iq == "buf" else None, iq_off), nsamples, f, None if null_p else C.byref(rp),
                                       nout, P(bufs["out"] if out == "buf" else None, out_off), out_stride, s)


def replay_argument_errors(V, torch):
    """-> the number of cases checked; what is allowed is called too, and nothing but the named outputs is written"""
    bufs = dict(iq=torch.zeros(2 * 4096 + 8, dtype=torch.float32, device="cuda"),
                taps=torch.zeros(16384 + 8, dtype=torch.float32, device="cuda"),
                nco=torch.zeros(2 * 256 + 8, dtype=torch.float32, device="cuda"),
                out=torch.full((2 * 16 * 128 + 8,), 7.0, dtype=torch.float32, device="cuda"))
    cases = argument_error_cases()
    for what, kw in cases:
        assert resample_call(V, torch, bufs, **kw) == 1, what
        assert "bad arguments" in V.last_error(), what
    assert resample_call(V, torch, bufs, nout=0) == 0
    assert resample_call(V, torch, bufs, nout=0, nsamples=0, out_stride=0) == 0
    torch.cuda.synchronize()
    assert bool((bufs["out"] == 7.0).all())
    # what is allowed: an integer format at 4 bytes, a scale that float32 ignores, nco_bits unread without rot, 16 channels,
    # exactly the count, out_stride = nout, out_stride < nout with one channel, L and M not coprime
    ok = [dict(iq_off=4, fmt=(2, 1.0)), dict(fmt=(0, float("nan"))), dict(rot=None, nco=None, par=dict(nchan=1, nco_bits=0)),
          dict(par=dict(nchan=16)), dict(nout="count", nsamples=240), dict(out_stride=100),
          dict(par=dict(nchan=1), out_stride=0), dict(par=dict(L=6, M=14)), dict(par=dict(L=128, M=4096, T=128), nout=1)]
    for kw in ok:
        assert resample_call(V, torch, bufs, **kw) == 0, (kw, V.last_error())
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        V.iq_resample_dev(bufs["iq"], 3, 7, bufs["taps"][:24].view(3, 8), 100, bufs["out"][:100])
    with pytest.raises(ValueError):
        V.iq_resample_dev(bufs["iq"], 3, 7, bufs["taps"][:24].view(4, 6), 100, bufs["out"])
    with pytest.raises(ValueError):
        V.iq_resample_dev(bufs["iq"], 3, 7, bufs["taps"][:24].view(3, 8), 100, bufs["out"], nsamples=5000)
    return len(cases)


def test_resample_calls_fail_loudly(V):
    """without a device: VIT_ERR_NO_DEVICE first, whatever the arguments, and an error text naming gfx950 - nothing is
    launched; the host helpers work without one.  With one, every argument rule is VIT_ERR_ARG"""
    import torch
    if torch.cuda.is_available():
        assert replay_argument_errors(V, torch) >= 35
        return
    good = V.ResampleParams(512, 625, 32, 1, 0, None, None, 0, 0, None)
    bad = V.ResampleParams(0, 0, 3, 99, 0, None, None, 77, 1, None)
    for p in (C.byref(good), C.byref(bad), None):
        assert V.lib().vit_iq_resample_dev(None, 0, None, p, 1, None, 0, None) == 2
        assert "gfx950" in V.last_error()
    assert V.lib().vit_iq_resample_dev(None, 100, C.byref(V.IqFormat(9, 0.0)), None, -1, None, 0, None) == 2
    assert V.resample_out_count(2500, 512, 625, 32) == out_count_model(2500, 512, 625, 32) > 0
