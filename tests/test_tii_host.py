"""CPU-only: "Transmitter identification" (include/viterbi_amd.h) - the definition of vit_ofdm_tii_dev as a numpy float32
model independent of the library (tii_model: the window through convert_model / rotate_model / fft_model, every sum an
explicit binary32 loop in the header's order, the noise level by rank counting) and the same estimator in float64
(tii_f64).  The streams are those of tests/test_sync_host.py's transmitter with a TII null symbol written into the silence
in front of every frame (add_null_symbols).  The model is pinned against the transmitted (mask, c) sets without noise and
with it, against tii_f64, and behind sync_model on frames with a carrier offset; the two host helpers against their rules.
tests/test_gpu_tii.py uses tii_model as its exact reference."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from test_fft_host import F32, U, fft_model, nco_model, rotate_model, twiddles_model
from test_iqfmt_host import IQ_CS8, IQ_CU8, convert_model, quantise
from test_sync_host import Params, prs_table, split, std_bins, sync_model, transmit_frames


class Tii:
    """vit_tii_params"""

    def __init__(self, nfft, Gp, C, R, navg=8, thr=2.5, offset=0):
        self.nfft, self.Gp, self.C, self.R, self.navg, self.thr, self.offset = nfft, Gp, C, R, navg, thr, offset

    def ngrp(self, nframes):
        return -(-nframes // self.navg)


# ---- the definition -------------------------------------------------------------------------------------------------

def serial_sum(terms):
    """terms: a sequence of float32 arrays of one shape -> their sum in ascending order in ONE accumulator from +0"""
    terms = list(terms)
    acc = np.zeros(terms[0].shape, F32)
    with np.errstate(all="ignore"):
        for v in terms:
            assert v.dtype == F32
            acc = acc + v
    assert acc.dtype == F32
    return acc


def rank_select(v, want):
    """the value of 0-based ascending rank `want` of a 1-D array, by the rule of the kernel: an element's rank is the
    number of smaller values plus the number of equal values with a lower index"""
    v = np.asarray(v)
    idx = np.arange(v.size)
    rank = (v[None, :] < v[:, None]).sum(axis=1) + ((v[None, :] == v[:, None]) & (idx[None, :] < idx[:, None])).sum(axis=1)
    assert sorted(rank.tolist()) == list(range(v.size))
    return v[rank == want][0]


def decide_model(E, thr):
    """E: float32 (Gp, C) -> (noise float32, mask uint32 (C,), strength float32 (C,))"""
    assert E.dtype == F32
    Gp, C_ = E.shape
    noise = rank_select(E.reshape(-1), (Gp * C_ - 1) // 2)
    with np.errstate(all="ignore"):
        tau = F32(thr) * noise
        on = (E > 0) & (E >= tau)
        mask = np.zeros(C_, np.uint32)
        strength = np.zeros(C_, F32)
        for b in range(Gp):
            mask |= on[b].astype(np.uint32) << np.uint32(b)
            strength = np.where(on[b], strength + E[b], strength)
    assert strength.dtype == F32 and noise.dtype == F32
    return noise, mask, strength


def pair_power_model(X, pairs, p):
    """X: complex64 (nfft,) -> f float32 (Gp*C,): e of every pair, summed over r in ascending r"""
    re, im = split(X)
    k = np.minimum(np.asarray(pairs, np.int64).reshape(p.R, p.Gp * p.C), p.nfft - 2)
    with np.errstate(all="ignore"):
        pw = re * re + im * im
        return serial_sum(pw[k[r]] + pw[k[r] + 1] for r in range(p.R))


def tii_model(x, starts, p, pairs, tw, nco=None, nco_bits=0, rot=None, fmt=None, nsamples=None):
    """x: the samples - complex64 (n,), or with fmt = (format, scale) the raw (n, 2) integers; starts: the frames' starts
    (with a stride: t*frame_stride); rot: (nframes, 2) of phase0, step, or None -> (words uint32 (ngrp, 2 + 2C), energy
    float32 (ngrp, Gp, C)).  Samples at and beyond nsamples belong to the buffer only."""
    n = len(x) if nsamples is None else nsamples
    nframes = len(starts)
    words = np.zeros((p.ngrp(nframes), 2 + 2 * p.C), np.uint32)
    energy = np.zeros((p.ngrp(nframes), p.Gp, p.C), F32)
    for g in range(p.ngrp(nframes)):
        rows = []
        for t in range(g * p.navg, min((g + 1) * p.navg, nframes)):
            s = int(starts[t])
            w0 = s + p.offset
            if s < 0 or w0 < 0 or w0 + p.nfft > n:
                continue
            win = x[w0:w0 + p.nfft]
            win = np.asarray(win, np.complex64) if fmt is None else convert_model(win, fmt[0], fmt[1])
            win = win.reshape(1, 1, p.nfft)
            if rot is not None:
                ph0, step = int(rot[t][0]), int(rot[t][1])
                # n = offset + i enters the phase mod 2^32: phase0 + (offset + i)*step = (phase0 + offset*step) + i*step
                win = rotate_model(win, nco, nco_bits, [[(ph0 + (p.offset % (1 << 32)) * step) % (1 << 32), step]], 0)
            rows.append(pair_power_model(fft_model(win, tw)[0, 0], pairs, p))
        E = (serial_sum(rows) if rows else np.zeros(p.Gp * p.C, F32)).reshape(p.Gp, p.C)
        noise, mask, strength = decide_model(E, p.thr)
        energy[g] = E
        words[g, 0] = len(rows)
        words[g, 1] = noise.view(np.uint32)
        words[g, 2::2] = mask
        words[g, 3::2] = strength.view(np.uint32)
    return words, energy


def masks_of(words):
    return words[:, 2::2]


def tii_f64(x, starts, p, pairs, steps=None):
    """the same estimator in float64 with np.fft -> masks uint32 (ngrp, C)"""
    x = np.asarray(x, np.complex128)
    k = np.minimum(np.asarray(pairs, np.int64).reshape(p.R, p.Gp * p.C), p.nfft - 2)
    out = np.zeros((p.ngrp(len(starts)), p.C), np.uint32)
    for g in range(out.shape[0]):
        E = np.zeros(p.Gp * p.C)
        for t in range(g * p.navg, min((g + 1) * p.navg, len(starts))):
            w0 = int(starts[t]) + p.offset
            if starts[t] < 0 or w0 < 0 or w0 + p.nfft > x.size:
                continue
            win = x[w0:w0 + p.nfft]
            if steps is not None:
                s = int(steps[t]) - (1 << 32) if int(steps[t]) >= 1 << 31 else int(steps[t])
                win = win * np.exp(2j * np.pi * s / 2.0 ** 32 * (p.offset + np.arange(p.nfft)))
            pw = np.abs(np.fft.fft(win)) ** 2
            E += (pw[k] + pw[k + 1]).sum(axis=0)
        noise = np.sort(E)[(E.size - 1) // 2]
        on = ((E > 0) & (E >= p.thr * noise)).reshape(p.Gp, p.C)
        out[g] = (on.astype(np.uint32) << np.arange(p.Gp, dtype=np.uint32)[:, None]).sum(axis=0)
    return out


# ---- the tables and the streams -------------------------------------------------------------------------------------

def pair_bins_model(mode=1):
    """the rule of vit_tii_pair_bins for mode I -> uint16 (4, 8, 24)"""
    assert mode == 1
    base = np.array([-768, -384, 1, 385])
    k0 = base[:, None, None] + 48 * np.arange(8)[None, :, None] + 2 * np.arange(24)[None, None, :]
    return (k0 % 2048).astype(np.uint16)


def random_pairs(rng, nfft, Gp, C_, R):
    """R*Gp*C non-overlapping pairs anywhere in the spectrum, bin nfft-1 never the lower one -> uint16 (R, Gp, C)"""
    odd = int(rng.integers(0, 2))
    lower = 2 * rng.permutation(nfft // 2 - odd)[:R * Gp * C_] + odd
    assert lower.size == R * Gp * C_ and np.unique(np.concatenate([lower, lower + 1])).size == 2 * lower.size and lower.max() + 1 < nfft
    return lower.reshape(R, Gp, C_).astype(np.uint16)


MAIN_WORDS = [w for w in range(256) if bin(w).count("1") == 4]  # ascending: p is the index


def mask_of_main_id(pid):
    """the mask (bit b = group b) of main identifier p: its pattern word with group 0 in the most significant bit"""
    w = MAIN_WORDS[pid]
    return sum((w >> (7 - b) & 1) << b for b in range(8))


def add_null_symbols(rng, x, true, prm, p, pairs, txs, amp, offsets=None, null_len=None, every_second=False):
    """writes a TII null symbol into the silence in front of every frame of transmit_frames' stream x (true: the frames'
    true starts): the carrier pairs of every (mask, c) of txs at amplitude amp and random phases, cyclically extended to
    null_len samples that end where the reference symbol's guard begins, under the frame's own frequency offset
    (offsets[t] carrier spacings, its phase continuous into the frame) - optionally in every second frame only"""
    nfft, G = prm.nfft, prm.guard
    null_len = prm.sym_stride + prm.W + 8 if null_len is None else null_len
    pairs = np.asarray(pairs, np.int64).reshape(p.R, p.Gp, p.C)
    y = np.asarray(x, np.complex128).copy()
    for t, s in enumerate(int(v) for v in true):
        if every_second and t % 2:
            continue
        Z = np.zeros(nfft, np.complex128)
        for mask, c in txs:
            for b in range(p.Gp):
                if mask >> b & 1:
                    k = pairs[:, b, c]
                    Z[k] += amp * np.exp(2j * np.pi * rng.random(p.R))
                    Z[k + 1] += amp * np.exp(2j * np.pi * rng.random(p.R))
        sym = np.fft.ifft(Z)  # the stream's scale is 1/nfft: the FFT of the window gives Z back
        n = np.arange(-null_len, 0)  # counted from the first sample of the reference symbol's guard
        cfo = 0.0 if offsets is None else offsets[t]
        assert s - G - null_len >= 0
        y[s - G - null_len:s - G] += sym[n % nfft] * np.exp(2j * np.pi * cfo * n / nfft)  # sample s - G - nfft is sym[0]
    return y.astype(np.complex64)


def tii_stream(rng, prm, p, pairs, txs, nframes, snr_db=None, tii_db=6.0, offsets=None, every_second=False):
    """nframes frames of prm behind TII null symbols -> (x complex64, true starts); with noise the TII carriers lie tii_db
    above the noise in an FFT bin, without it they have the data carriers' amplitude"""
    bins = std_bins(prm.nfft)
    prs = prs_table(rng, prm.nfft, bins)
    null_len = prm.sym_stride + prm.W + 8
    offsets = [0.0] * nframes if offsets is None else offsets
    x, true, _ = transmit_frames(rng, prm, prs, bins, nframes, offsets, lead=[null_len + 4] * nframes, snr_db=snr_db)
    amp = 1.0 if snr_db is None else 10.0 ** ((tii_db - snr_db) / 20.0)
    return add_null_symbols(rng, x, true, prm, p, pairs, txs, amp, offsets, null_len, every_second), true, prs


def expected_masks(p, txs):
    want = np.zeros(p.C, np.uint32)
    for mask, c in txs:
        want[c] |= np.uint32(mask)
    return want


# ---- the model's parts ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", (4, 8 * 256))
def test_serial_sum_against_float64(n):
    """n non-negative terms in one accumulator: relative error at most gamma_(n-1) = (n-1)u / (1 - (n-1)u) (Higham,
    Accuracy and Stability of Numerical Algorithms, eq. 4.4 - every term passes through at most n-1 additions); and the
    order is observable: 2^24 absorbs ones added after it, not before it"""
    rng = np.random.default_rng(n)
    v = (rng.random((n, 50)) * 2.0 ** rng.integers(-20, 20, (n, 50))).astype(F32)
    got = serial_sum(v).astype(np.float64)
    ref = v.astype(np.float64).sum(axis=0)
    gamma = (n - 1) * U / (1 - (n - 1) * U)
    err = np.abs(got - ref) / ref
    print("n", n, "max relative error", err.max(), "bound", gamma)
    assert (err <= gamma).all()
    ones = [np.array([2.0 ** 24], F32)] + [np.array([1.0], F32)] * 8
    assert serial_sum(ones)[0] == F32(2.0 ** 24) and serial_sum(ones[::-1])[0] == F32(2.0 ** 24 + 8)


def test_rank_rule_with_ties_and_zeros():
    """the rank rule is a selection: whatever ties and zeros there are, it returns what sorting returns, for every rank"""
    rng = np.random.default_rng(1)
    cases = [np.zeros(7, F32), np.array([3, 1, 3, 0, 0, 1, 3, 2], F32), np.array([5], F32), np.array([2, 2], F32),
             rng.integers(0, 4, 48).astype(F32), rng.random(33).astype(F32), np.array([0, 0, 0, 1, 0, 0], F32)]
    for v in cases:
        for want in range(v.size):
            assert rank_select(v, want) == np.sort(v)[want]
    # the lower median of an even count: the smaller of the two middle values; all zeros but one: 0
    E = np.array([[4, 1], [3, 2]], F32)
    assert decide_model(E, 1.0)[0] == 2.0
    noise, mask, strength = decide_model(np.array([[0, 0, 9], [0, 0, 0]], F32), 2.5)
    assert noise == 0 and mask.tolist() == [0, 0, 1] and strength.tolist() == [0, 0, 9]  # E > 0 decides where tau is 0


def test_decision_edges():
    """a slot exactly at tau is on, strength sums in ascending b in one accumulator, all-zero energies give nothing"""
    E = np.array([[1.0, 4.0, 2.5], [1.0, 1.0, 2.4999998]], F32)  # lower median of 6 values: rank 2 -> 1.0
    noise, mask, strength = decide_model(E, 2.5)
    assert noise == 1.0 and mask.tolist() == [0, 1, 1] and strength.tolist() == [0.0, 4.0, 2.5]
    E = np.zeros((9, 2), F32)
    E[:, 1] = [2.0 ** 24] + [1.0] * 8  # ascending b: the ones are lost one by one
    E[0, 0] = 1.0
    noise, mask, strength = decide_model(E, 1.0)
    assert noise == 1.0 and mask.tolist() == [1, 0x1FF] and strength[1] == F32(2.0 ** 24)
    noise, mask, strength = decide_model(np.zeros((8, 24), F32), 2.5)
    assert noise == 0 and not mask.any() and not strength.any()


# ---- the model against the truth --------------------------------------------------------------------------------------

MODE_I_LIKE = dict(nfft=2048, guard=504, nsyms=2, W=8, M=2)  # mode I's symbol, a frame of two symbols
# The threshold of the noise-free tests.  Without noise the level under the median is the float32 transform's own
# rounding, and all that is known of it is an upper bound: the relative L2 error of fft_model is at most 8 m u
# (tests/test_fft_host.py, after Higham), so at nfft 2048 ALL unsent slots together hold at most (8 * 11 * 2^-24)^2 =
# 2^-35.1 of the window's power, while each of the at most 12 sent slots (equal amplitudes) holds 1/12 of it: a sent slot
# lies 2^31.5 (95 dB) or more above every unsent one and above the median.  The rounding is not white - the butterflies'
# errors follow the sparse spectrum, and slots a power of two of carriers away from a sent pair hold 40 times the
# median, so the receiver's thr of 2.5, which is made for a noise level, would set bits there (measured: combs c + 8
# and c + 16 get all eight).  The tests take the middle of the guaranteed gap in dB, 2^16: every sent bit is then
# guaranteed by the bound, and an unsent bit would need rounding errors 48 dB apart inside one transform.
NOISE_FREE_THR = 2.0 ** 16


def std_case(navg=8, thr=NOISE_FREE_THR):
    prm = Params(**MODE_I_LIKE)
    return prm, Tii(2048, 8, 24, 4, navg=navg, thr=thr, offset=-prm.sym_stride), pair_bins_model()


@pytest.mark.parametrize("txs", [[(7, 3)], [(0, 0), (69, 23)], [(12, 5), (40, 6), (55, 17)]], ids=("1", "2", "3"))
def test_noise_free_transmitters(V, txs):
    """1, 2 and 3 transmitters (main id, sub id) with distinct sub ids, mode I's table, 8 frames: every transmitted mask
    exact, every other mask 0, and vit_tii_main_id returns the main ids (thr: NOISE_FREE_THR above)"""
    prm, p, pairs = std_case()
    rng = np.random.default_rng(100 + len(txs))
    sent = [(mask_of_main_id(pid), c) for pid, c in txs]
    x, true, _ = tii_stream(rng, prm, p, pairs, sent, 8)
    words, energy = tii_model(x, true, p, pairs, twiddles_model(2048))
    assert words[0, 0] == 8 and np.array_equal(masks_of(words)[0], expected_masks(p, sent))
    for pid, c in txs:
        assert V.tii_main_id(int(masks_of(words)[0, c])) == pid
    assert np.array_equal(tii_f64(x, true, p, pairs), masks_of(words))
    rec = V.tii_records(words, p.C)
    assert rec["nused"].tolist() == [8] and np.array_equal(rec["comb"]["mask"], masks_of(words))
    assert rec["noise"][0] == words[0, 1:2].view(F32)[0] and rec["comb"]["strength"][0, txs[0][1]] > 0


def test_two_transmitters_share_a_comb(V):
    """the union of two patterns: popcount > 4, vit_tii_main_id answers -1"""
    prm, p, pairs = std_case()
    rng = np.random.default_rng(104)
    sent = [(mask_of_main_id(0), 9), (mask_of_main_id(69), 9)]
    x, true, _ = tii_stream(rng, prm, p, pairs, sent, 8)
    words, _ = tii_model(x, true, p, pairs, twiddles_model(2048))
    assert masks_of(words)[0, 9] == 0xFF and not np.delete(masks_of(words)[0], 9).any()
    assert V.tii_main_id(0xFF) == -1
    sent = [(mask_of_main_id(3), 9), (mask_of_main_id(4), 9)]
    x, true, _ = tii_stream(rng, prm, p, pairs, sent, 8)
    m = int(masks_of(tii_model(x, true, p, pairs, twiddles_model(2048))[0])[0, 9])
    assert m == sent[0][0] | sent[1][0] and bin(m).count("1") > 4 and V.tii_main_id(m) == -1


# (nfft, Gp, C, R), the transmitters as (mask, c), every second frame only
NOISE_LAYOUTS = [((2048, 8, 24, 4), [(0x0F, 2), (0xA5, 11), (0xC3, 20)], False),
                 ((256, 8, 3, 4), [(0x3C, 1)], False),
                 ((256, 8, 3, 4), [(0x3C, 0), (0x99, 2)], False),
                 ((512, 8, 6, 2), [(0x0F, 1), (0x5A, 4)], False),
                 ((2048, 8, 24, 4), [(0x0F, 2), (0xA5, 11), (0xC3, 20)], True),
                 ((256, 8, 3, 4), [(0x3C, 0), (0x99, 2)], True)]


@pytest.mark.parametrize("layout,txs,second", NOISE_LAYOUTS)
def test_noise_every_bit_and_no_other(layout, txs, second):
    """TII carriers 6 dB above the noise of an FFT bin (data carriers at 10 dB), navg 8, thr 2.5 - with TII in every
    second frame only: thr 2.0 -, fewer than half of the slots occupied: in every group the model finds every transmitted
    bit and no other, and the float64 estimator agrees on every mask"""
    nfft, Gp, C_, R = layout
    assert sum(bin(m).count("1") for m, _ in txs) < Gp * C_ // 2
    rng = np.random.default_rng(200 + nfft + C_ + len(txs) + second)
    prm = Params(nfft, nfft // 4, 2, 8, 2)
    p = Tii(nfft, Gp, C_, R, navg=8, thr=2.0 if second else 2.5, offset=-prm.sym_stride)
    pairs = pair_bins_model() if nfft == 2048 else random_pairs(rng, nfft, Gp, C_, R)
    ngroups = 3
    x, true, _ = tii_stream(rng, prm, p, pairs, txs, 8 * ngroups, snr_db=10.0, every_second=second)
    words, energy = tii_model(x, true, p, pairs, twiddles_model(nfft))
    want = expected_masks(p, txs)
    print("noise", words[:, 1].view(F32).tolist(), "weakest sent slot / noise",
          [float(min(energy[g, b, c] for m, c in txs for b in range(Gp) if m >> b & 1) / words[g, 1:2].view(F32)[0])
           for g in range(ngroups)])
    assert (words[:, 0] == 8).all()
    for g in range(ngroups):
        assert np.array_equal(masks_of(words)[g], want), g
    assert np.array_equal(tii_f64(x, true, p, pairs), masks_of(words))


def test_carrier_offset_needs_the_rotation():
    """3 carrier spacings of offset: the pairs lie 3 bins away, the masks are wrong without d_rot and right with the
    tables sync_model writes - the window is counted from ITS start, the rotation's n runs negative"""
    nfft, G = 256, 64
    prm = Params(nfft, G, 4, 6, 4, backoff=5)
    p = Tii(nfft, 8, 3, 4, navg=4, thr=2.5, offset=-prm.sym_stride)
    rng = np.random.default_rng(300)
    pairs = random_pairs(rng, nfft, 8, 3, 4)
    txs = [(0x3C, 0), (0x99, 2)]
    offsets = [3.0, 3.2, 2.7, 3.0]
    x, true, prs = tii_stream(rng, prm, p, pairs, txs, 4, snr_db=20.0, tii_db=10.0, offsets=offsets)
    tw, nco = twiddles_model(nfft), nco_model(14)
    start, rot, _, _ = sync_model(x, true - 3, prm, prs, tw, nco, 14)
    assert np.array_equal(start, true - prm.backoff)
    want = expected_masks(p, txs)
    plain = masks_of(tii_model(x, start, p, pairs, tw)[0])[0]
    assert not np.array_equal(plain, want)
    words, _ = tii_model(x, start, p, pairs, tw, nco, 14, rot)
    assert words[0, 0] == 4 and np.array_equal(masks_of(words)[0], want)
    assert np.array_equal(tii_f64(x, start, p, pairs, rot[:, 1])[0], want)


def test_skip_rule_ragged_groups_and_zero_windows():
    """start -1, a window cut by either end of the buffer, a group with nused 0, a ragged last group; all-zero windows;
    an entry nfft-1 in the pair table reads bins nfft-2 and nfft-1"""
    nfft = 64
    rng = np.random.default_rng(400)
    p = Tii(nfft, 4, 3, 2, navg=3, thr=1.5, offset=-10)
    pairs = random_pairs(rng, nfft, 4, 3, 2)
    x = (rng.standard_normal(700) + 1j * rng.standard_normal(700)).astype(np.complex64)
    tw = twiddles_model(nfft)
    #         cut in front, whole, -1 | all three skipped | whole, cut behind (ends at 701), whole to the last sample | whole
    starts = [9, 10, -1, -1, 5, 700, 100, 647, 646, 300]
    words, energy = tii_model(x, starts, p, pairs, tw)
    assert words.shape == (4, 8) and words[:, 0].tolist() == [1, 0, 2, 1]
    assert not words[1].any() and not energy[1].any()
    one = tii_model(x, [10], p, pairs, tw)
    assert np.array_equal(one[0][0], words[0]) and np.array_equal(one[1][0], energy[0])
    two = tii_model(x, [100, 646], p, pairs, tw)
    assert np.array_equal(two[0][0], words[2]) and np.array_equal(tii_model(x, [300], p, pairs, tw)[0][0], words[3])
    # nsamples in front of the buffer's end: what lies behind it is not read
    y = x.copy()
    y[690:] = np.nan
    assert np.array_equal(tii_model(y, starts, p, pairs, tw, nsamples=690)[0], tii_model(x[:690], starts, p, pairs, tw)[0])
    # all-zero windows: noise 0, every mask 0, nused counts them
    z = np.zeros(300, np.complex64)
    words, energy = tii_model(z, [10, 80, 150], p, pairs, tw)
    assert words[0].tolist() == [3] + [0] * 7 and not energy.any()
    # the clamp
    q = pairs.copy()
    q[1, 2, 1] = nfft - 1
    r = pairs.copy()
    r[1, 2, 1] = nfft - 2
    a, b = tii_model(x, [10, 100], p, q, tw), tii_model(x, [10, 100], p, r, tw)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(a[1], tii_model(x, [10, 100], p, pairs, tw)[1])


def test_integer_formats_in_the_model():
    """an integer stream is read as the floats of "Integer sample formats": the masks of a CS8 and a CU8 stream at 10 dB"""
    rng = np.random.default_rng(500)
    prm = Params(256, 64, 2, 8, 2)
    p = Tii(256, 8, 3, 4, navg=8, thr=2.5, offset=-prm.sym_stride)
    pairs = random_pairs(rng, 256, 8, 3, 4)
    txs = [(0x3C, 0), (0x99, 2)]
    x, true, _ = tii_stream(rng, prm, p, pairs, txs, 8, snr_db=10.0)
    for fmt in (IQ_CS8, IQ_CU8):
        raw, scale = quantise(x, fmt)
        words, _ = tii_model(raw, true, p, pairs, twiddles_model(256), fmt=(fmt, scale))
        assert words[0, 0] == 8 and np.array_equal(masks_of(words)[0], expected_masks(p, txs)), fmt


# ---- the host helpers -------------------------------------------------------------------------------------------------

def test_pair_bins(V):
    """mode I: 768 distinct bins, every pair inside the 1536 used carriers and off DC, no two pairs overlapping; no other
    mode has a table"""
    t = V.tii_pair_bins(1)
    assert t.shape == (4, 8, 24) and t.dtype == np.uint16 and np.array_equal(t, pair_bins_model())
    lower = t.reshape(-1).astype(np.int64)
    assert np.unique(lower).size == 768
    both = np.concatenate([lower, lower + 1])
    assert np.unique(both).size == 1536  # no overlap: the pairs tile the used carriers
    carrier = np.where(both >= 1024, both - 2048, both)
    assert (carrier != 0).all() and (np.abs(carrier) <= 768).all() and sorted(carrier.tolist()) == [k for k in range(-768, 769) if k]
    assert (np.where(lower >= 1024, lower - 2048, lower) != -1).all()  # no pair straddles DC
    buf = (C.c_uint16 * 768)()
    for mode in (0, 2, 5):
        assert V.lib().vit_tii_pair_bins(mode, buf) == -1
        with pytest.raises(ValueError):
            V.tii_pair_bins(mode)
    assert V.lib().vit_tii_pair_bins(1, None) == -1 and V.lib().vit_tii_pair_bins(1, buf) == 768


def test_main_id(V):
    """a bijection from the 70 four-of-eight masks onto 0 ... 69; group 0 is the pattern word's most significant bit, so
    p = 0 (word 0x0F) is groups 4 ... 7, mask 0xF0; -1 for every other mask"""
    four = [m for m in range(256) if bin(m).count("1") == 4]
    ids = [V.tii_main_id(m) for m in four]
    assert len(four) == 70 and sorted(ids) == list(range(70))
    assert V.tii_main_id(0xF0) == 0 and V.tii_main_id(0xE8) == 1 and V.tii_main_id(0x0F) == 69
    for pid in range(70):
        assert V.tii_main_id(mask_of_main_id(pid)) == pid
    word = lambda m: sum((m >> b & 1) << (7 - b) for b in range(8))  # noqa: E731
    assert [word(m) for _, m in sorted(zip(ids, four))] == MAIN_WORDS and MAIN_WORDS[1] == 0x17
    for m in range(256):
        if bin(m).count("1") != 4:
            assert V.tii_main_id(m) == -1
    for m in (256, 0x10F, 0xF00, 0x0F00000F, 0xFFFFFFFF, -1, 1 << 32):
        assert V.tii_main_id(m) == -1


# ---- the library without a GPU --------------------------------------------------------------------------------------

def test_tii_exports(V):
    out = subprocess.check_output(["nm", "-D", "--defined-only", V.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in ("vit_ofdm_tii_dev", "vit_tii_pair_bins", "vit_tii_main_id"):
        assert name in exported and name in V.EXPORTS
    P = V.TiiParams
    assert C.sizeof(P) == 32 and [getattr(P, f).offset for f, _ in P._fields_] == [0, 4, 8, 12, 16, 20, 24]
    assert callable(V.ofdm_tii_dev) and callable(V.tii_records)
    with pytest.raises(ValueError):
        V.tii_records(np.zeros(49, np.uint32), 24)


def argument_error_cases(V, torch):
    """every rule of vit_ofdm_tii_dev that is VIT_ERR_ARG, on a device: -> the number of cases checked"""
    L = V.lib()
    nfft, n = 64, 1024
    d_iq = torch.zeros(2 * n + 8, dtype=torch.float32, device="cuda")
    d_tw = torch.from_numpy(V.fft_twiddles(nfft)).cuda()
    d_nco = torch.from_numpy(V.nco_table(8)).cuda()
    d_start = torch.tensor([100, 300, 500, 0], dtype=torch.int64, device="cuda")
    d_rot = torch.zeros(10, dtype=torch.int32, device="cuda")
    d_pairs = torch.from_numpy((2 * np.arange(26)).astype(np.int16)).cuda()
    d_tii = torch.full((40,), 7, dtype=torch.int32, device="cuda")
    d_en = torch.full((50,), 7.0, dtype=torch.float32, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731

    def call(inp=None, fmt=None, par=None, pairs=P(d_pairs), nframes=3, tii=P(d_tii), en=P(d_en), null_in=False, null_p=False):
        i = dict(d_iq=d_iq.data_ptr(), nsamples=n, sym_stride=0, frame_stride=0, d_start=d_start.data_ptr(), d_tw=d_tw.data_ptr(),
                 d_nco=d_nco.data_ptr(), nco_bits=8, d_rot=d_rot.data_ptr())
        i.update(inp or {})
        a = V.IqInput()
        for k, v in i.items():
            setattr(a, k, v)
        p = dict(nfft=nfft, ngroups=4, ncombs=3, nrep=2, navg=2, thr=2.5, offset=-20)
        p.update(par or {})
        tp = V.TiiParams(*[p[f] for f, _ in V.TiiParams._fields_])
        f = None if fmt is None else C.byref(V.IqFormat(*fmt))
        return L.vit_ofdm_tii_dev(None if null_in else C.byref(a), f, None if null_p else C.byref(tp), pairs, nframes, tii, en, s)

    inf, nan = float("inf"), float("nan")
    at = lambda t, off: t.data_ptr() + off  # noqa: E731
    bad = [dict(null_in=True), dict(null_p=True), dict(inp=dict(d_iq=None)), dict(inp=dict(d_tw=None)), dict(pairs=None),
           dict(tii=None), dict(nframes=-1),
           dict(inp=dict(d_iq=at(d_iq, 4))), dict(inp=dict(d_iq=at(d_iq, 2)), fmt=(V.IQ_CU8, 1.0)),
           dict(inp=dict(d_iq=at(d_iq, 2)), fmt=(V.IQ_CS16, 1.0)),
           dict(inp=dict(d_tw=at(d_tw, 4))), dict(inp=dict(d_nco=at(d_nco, 4))), dict(inp=dict(d_start=at(d_start, 4))),
           dict(inp=dict(d_rot=at(d_rot, 4))), dict(pairs=P(d_pairs, 1)), dict(tii=P(d_tii, 2)), dict(en=P(d_en, 2)),
           dict(par=dict(nfft=32)), dict(par=dict(nfft=96)), dict(par=dict(nfft=16384)), dict(par=dict(nfft=0)),
           dict(par=dict(ngroups=0)), dict(par=dict(ngroups=33, ncombs=1, nrep=1)), dict(par=dict(ncombs=0)),
           dict(par=dict(nfft=8192, ngroups=32, ncombs=33, nrep=1)),  # Gp*C = 1056
           dict(par=dict(nrep=0)), dict(par=dict(nrep=9, ngroups=1, ncombs=1)),
           dict(par=dict(nrep=3)),  # 2*3*12 = 72 > 64
           dict(par=dict(navg=0)), dict(par=dict(navg=257)),
           dict(par=dict(thr=0.0)), dict(par=dict(thr=-1.0)), dict(par=dict(thr=inf)), dict(par=dict(thr=nan)),
           dict(inp=dict(d_nco=None)), dict(inp=dict(nco_bits=0)), dict(inp=dict(nco_bits=21)),
           dict(fmt=(4, 1.0)), dict(fmt=(V.IQ_CU8, 0.0)), dict(fmt=(V.IQ_CS8, nan)), dict(fmt=(V.IQ_CS16, 2.0 ** 17)),
           # without the table every window must lie inside the buffer
           dict(inp=dict(d_start=None, frame_stride=100)),  # offset -20: frame 0's window starts in front of the buffer
           dict(inp=dict(d_start=None, frame_stride=481), par=dict(offset=0)),  # 2*481 + 64 = 1026 > 1024
           dict(inp=dict(d_start=None, frame_stride=0), par=dict(offset=n - nfft + 1)),
           dict(inp=dict(d_start=None, frame_stride=1 << 63), par=dict(offset=0))]
    for kw in bad:
        assert call(**kw) == 1, kw
        assert "bad arguments" in V.last_error(), kw
    assert call(nframes=0) == 0
    torch.cuda.synchronize()
    assert bool((d_tii == 7).all()) and bool((d_en == 7).all())
    # what is allowed: no d_energy, no rotation (then d_nco and nco_bits are not looked at), an integer format at 4 bytes,
    # a scale that F32 ignores, any finite thr, the struct's largest values, windows that end with the buffer
    no_rot = dict(d_rot=None, d_nco=None, nco_bits=0)
    assert call() == 0 and call(en=None) == 0 and call(inp=no_rot) == 0
    assert call(inp=dict(d_iq=at(d_iq, 4)), fmt=(V.IQ_CS8, 1.0)) == 0 and call(fmt=(V.IQ_F32, nan)) == 0
    assert call(par=dict(thr=3.0e38)) == 0 and call(par=dict(thr=1.0e-45)) == 0
    assert call(par=dict(ngroups=32, ncombs=1, nrep=1, navg=256), nframes=1) == 0
    assert call(inp=dict(d_start=None, frame_stride=480), par=dict(offset=0)) == 0
    assert call(inp=dict(d_start=None, frame_stride=0), par=dict(offset=n - nfft)) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        V.ofdm_tii_dev(d_iq, nfft, 3, d_tw, d_pairs, d_tii, 4, 3, 2, 2)  # neither d_start nor frame_stride
    with pytest.raises(ValueError):
        V.ofdm_tii_dev(d_iq, nfft, 3, d_tw, d_pairs[:23], d_tii, 4, 3, 2, 2, d_start=d_start)
    with pytest.raises(ValueError):
        V.ofdm_tii_dev(d_iq, nfft, 3, d_tw, d_pairs, d_tii[:15], 4, 3, 2, 2, d_start=d_start)
    with pytest.raises(ValueError):
        V.ofdm_tii_dev(d_iq, nfft, 3, d_tw, d_pairs, d_tii, 4, 3, 2, 2, d_start=d_start, d_energy=d_en[:23])
    with pytest.raises(ValueError):
        V.ofdm_tii_dev(d_iq, nfft, 3, d_tw, d_pairs, d_tii, 4, 3, 2, 2, d_start=d_start, nsamples=n + 5)
    return len(bad)


def test_tii_call_fails_loudly(V):
    """without a device: VIT_ERR_NO_DEVICE first, whatever the arguments, and an error text naming gfx950 - nothing is
    launched; with one, every argument rule is VIT_ERR_ARG"""
    import torch
    if torch.cuda.is_available():
        assert argument_error_cases(V, torch) >= 40
        return
    par = V.TiiParams(2048, 8, 24, 4, 8, 2.5, -2552)
    bad = V.TiiParams(3, 0, 0, 0, 0, -1.0, 0)
    inp = V.IqInput()
    for i in (C.byref(inp), None):
        for p in (C.byref(par), C.byref(bad), None):
            assert V.lib().vit_ofdm_tii_dev(i, None, p, None, 1, None, None, None) == 2
            assert "gfx950" in V.last_error()
    assert V.lib().vit_ofdm_tii_dev(None, C.byref(V.IqFormat(9, 0.0)), None, None, -1, None, None, None) == 2
