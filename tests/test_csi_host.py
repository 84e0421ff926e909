"""CPU-only: "Channel-state weighting" (include/viterbi_amd.h) - the per-symbol soft-decision rule as a numpy float32
model independent of the library (level_model: the level's summation grouping; demap_soft_model: the bytes), pinned by
its properties, by the order of its sum and by what it is for: the FIBs a two-path channel costs the per-carrier rule.
tests/test_gpu_csi.py uses the same model as its bit-exact reference.

Run as a script it prints the table of INTEGRATION.md 2i (bit errors / bad FIBs per rule and gain)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from test_ofdm_host import (MODE_I, MODE_III, demap_model, fic_bits, fic_decode, freq_bins_model, small_case,
                            special_carriers, transmit)

F32 = np.float32
SOFT_PER_CARRIER, SOFT_PER_SYMBOL = 0, 1
S_MIN, S_MAX = F32(2.0 ** -64), F32(2.0 ** 96)


# ---- the definition -------------------------------------------------------------------------------------------------

def level_model(v, nfft):
    """v: (..., K) float32 terms (nrm or +0) -> (...) float32 S, every addition one float32 operation in the header's
    grouping: groups of 4 in adjacent pairs, A = max(64, nfft/8) accumulators that take group i, i + A, ... in this
    order, then the tree of adjacent pairs"""
    v = np.asarray(v)
    assert v.dtype == F32
    K = v.shape[-1]
    G, A = -(-K // 4), max(64, nfft // 8)
    vv = np.zeros(v.shape[:-1] + (4 * G,), F32)
    vv[..., :K] = v
    g = vv.reshape(v.shape[:-1] + (G, 4))
    with np.errstate(over="ignore"):
        q = (g[..., 0] + g[..., 1]) + (g[..., 2] + g[..., 3])
        acc = np.zeros(v.shape[:-1] + (A,), F32)
        acc[..., :min(G, A)] = q[..., :A]
        for r in range(1, -(-G // A)):
            m = min(G - r * A, A)
            acc[..., :m] = acc[..., :m] + q[..., r * A:r * A + m]
        while acc.shape[-1] > 1:
            acc = acc[..., 0::2] + acc[..., 1::2]
    assert acc.dtype == F32
    return acc[..., 0]


def demap_soft_model(z, bins, shape, gain):
    """z: (nframes, nsyms, nfft) complex64 FFT outputs -> (soft bytes (nframes, nsyms-1, 2K), levels (nframes, nsyms-1)
    float32) of VIT_SOFT_PER_SYMBOL; every operation one numpy float32 operation in the order of the header"""
    nfft, K, nsyms = shape[0], shape[1], shape[2]
    z = np.asarray(z, np.complex64).reshape(-1, nsyms, nfft)[:, :, np.asarray(bins, np.int64)]
    assert z.shape[2] == K
    ar, ai, br, bi = z.real[:, 1:], z.imag[:, 1:], z.real[:, :-1], z.imag[:, :-1]
    with np.errstate(all="ignore"):
        re = ar * br + ai * bi
        im = ai * br - ar * bi
        nrm = np.abs(re) + np.abs(im)
        ok = (nrm >= F32(2.0 ** -64)) & (nrm <= np.finfo(F32).max)
        S = level_model(np.where(ok, nrm, F32(0)), nfft)
        sok = (S >= S_MIN) & (S <= S_MAX)
        s = ((F32(gain) * F32(K)) / np.where(sok, S, F32(1)))[..., None]
        assert re.dtype == F32 and S.dtype == F32 and s.dtype == F32
        q0 = np.clip(F32(128) - np.rint(np.where(ok, re, F32(0)) * s), 0, 255)
        q1 = np.clip(F32(128) - np.rint(np.where(ok, im, F32(0)) * s), 0, 255)
    live = ok & sok[..., None]
    out = np.concatenate([np.where(live, q0, 128), np.where(live, q1, 128)], axis=2)
    return out.astype(np.uint8), S


# ---- the model's properties -----------------------------------------------------------------------------------------

def test_flat_channel_gives_half_the_gain():
    rng = np.random.default_rng(1)
    bins, bits = small_case(rng)
    z = transmit(bits, bins, MODE_III, rng)
    for gain in (16.0, 64.0, 128.0, 254.0, 2.0):
        out, S = demap_soft_model(z, bins, MODE_III, gain)
        assert np.array_equal(out > 128, bits.astype(bool)), gain
        ideal = np.where(bits == 1, 128 + gain / 2, 128 - gain / 2)
        assert np.abs(out.astype(np.float64) - np.clip(ideal, 0, 255)).max() <= 1, gain
        assert np.allclose(S, MODE_III[1] * np.sqrt(2.0), rtol=1e-5)  # |re| + |im| of a unit carrier on a diagonal


def test_soft_value_grows_with_the_square_of_the_amplitude():
    """a carrier at twice the mean amplitude: four times the excursion, until the clamp"""
    rng = np.random.default_rng(2)
    bins, bits = small_case(rng, MODE_III, 1)
    K = MODE_III[1]
    h = np.ones(256)
    h[bins[7]] = 2.0
    z = transmit(bits, bins, MODE_III, rng, carrier_gain=h)
    out, S = demap_soft_model(z, bins, MODE_III, 16.0)
    exc = np.abs(out.astype(int) - 128)
    others = np.delete(np.arange(K), 7)
    assert set(exc[0, :, others].ravel()) == {8}            # rint(8 K / (K + 3)) = 8
    assert np.abs(exc[0, :, 7] - 32).max() <= 1 and np.abs(exc[0, :, K + 7] - 32).max() <= 1
    assert np.array_equal(out > 128, bits.astype(bool))
    out, _ = demap_soft_model(z, bins, MODE_III, 128.0)     # 4 * 64 = 256: the clamp
    assert np.array_equal(out[0, :, 7], np.where(bits[0, :, 7] == 1, 255, 0))
    assert np.abs(np.abs(out[0, :, others].astype(int) - 128) - 63).max() <= 1


def test_special_carriers_are_erasures_and_leave_the_sum():
    """zero, 2^-70, NaN, Inf, mixed NaN and overflowing carriers are 128; the symbol's other carriers are exactly what
    they are when those carriers are zero (all are +0 in the sum), and differ from the undisturbed symbol by no more
    than the 6 removed terms change S"""
    rng = np.random.default_rng(3)
    bins, bits = small_case(rng)
    K = MODE_III[1]
    clean = transmit(bits, bins, MODE_III, rng)
    z, zeroed = clean.copy(), clean.copy()
    n = special_carriers(z, bins, 5)
    zeroed[:, 5, bins[:n]] = 0
    gain = 64.0
    out, S = demap_soft_model(z, bins, MODE_III, gain)
    out0, S0 = demap_soft_model(zeroed, bins, MODE_III, gain)
    outc, Sc = demap_soft_model(clean, bins, MODE_III, gain)
    for s in (4, 5):  # symbol 5 is `a` of data symbol 4 and `b` of data symbol 5
        assert (out[:, s, :n] == 128).all() and (out[:, s, K:K + n] == 128).all()
    assert np.array_equal(out, out0) and np.array_equal(S.view(np.uint32), S0.view(np.uint32))
    assert np.isfinite(S).all() and (S[:, 4:6] < Sc[:, 4:6]).all()
    assert np.array_equal(S[:, :4].view(np.uint32), Sc[:, :4].view(np.uint32)) and np.array_equal(out[:, 6:], outc[:, 6:])
    # excursion gain/2 = 32 grows by S_clean / S = K / (K - 6) at most: 32 * 6 / 186 = 1.03, plus one rounding each
    rest = np.r_[n:K, K + n:2 * K]
    assert np.abs(out[:, 4:6][:, :, rest].astype(int) - outc[:, 4:6][:, :, rest].astype(int)).max() <= 2
    assert np.array_equal(out[:, :, rest] > 128, bits[:, :, rest].astype(bool))


def test_silent_and_overdriven_symbols_are_all_erasures():
    rng = np.random.default_rng(4)
    bins, bits = small_case(rng)
    z = transmit(bits, bins, MODE_III, rng)
    z[:, 5] = 0                      # data symbols 4 and 5: every product is 0
    z[:, 9:11] *= F32(2.0 ** 45)     # data symbol 9: products of 2^90, K of them beyond 2^96; 8 and 10: 2^45, fine
    z[1, 20] *= F32(2.0 ** -40)      # data symbols 19 and 20 of frame 1: products of 2^-40, weak but no erasures
    out, S = demap_soft_model(z, bins, MODE_III, 64.0)
    assert (out[:, 4:6] == 128).all() and (S[:, 4:6] == 0).all()
    assert (out[:, 9] == 128).all() and np.isfinite(S[:, 9]).all() and (S[:, 9] > S_MAX).all()
    for s in (3, 6, 8, 10):
        assert np.array_equal(out[:, s] > 128, bits[:, s].astype(bool)) and (S[:, s] <= S_MAX).all()
    assert np.array_equal(out[1, 19:21] > 128, bits[1, 19:21].astype(bool)) and (S[1, 19:21] < 2.0 ** -30).all()
    # a level that overflows is +Inf, never NaN, and the symbol is all erasures
    z[:, 9:11] *= F32(2.0 ** 18)     # products of 2^126 and more: each finite, their sum is not
    out, S = demap_soft_model(z, bins, MODE_III, 64.0)
    assert np.isposinf(S[:, 9]).all() and (out[:, 9] == 128).all()


# ---- the order of the sum -------------------------------------------------------------------------------------------

GROUPING_SEED = 1  # found on the CPU: the three sums below differ on it


def grouping_terms():
    return np.random.default_rng(GROUPING_SEED).uniform(0.5, 2.0, 1536).astype(F32)


def test_the_grouping_is_the_header_s():
    """one fixed input on which the header's grouping, numpy's own float32 sum (pairwise in blocks) and a plain left-to-right
    sum give three different values; and the grouping written out again, with loops, gives the model's"""
    v = grouping_terms()
    S = level_model(v, 2048)
    plain = F32(0)
    for x in v:
        plain = plain + x
    assert plain.dtype == F32
    assert S != np.sum(v, dtype=F32) and S != plain, "choose another GROUPING_SEED"
    assert abs(float(S) - float(np.sum(v, dtype=np.float64))) < 1536 * 2.0 ** -22
    for nfft, K in ((2048, 1536), (64, 5), (64, 64), (256, 192), (512, 384), (1024, 1024), (8192, 8192), (128, 77)):
        w = np.random.default_rng(K).uniform(0.5, 2.0, K).astype(F32)
        G, A = -(-K // 4), max(64, nfft // 8)
        pad = np.concatenate([w, np.zeros(4 * G - K, F32)])
        acc = [F32(0)] * A
        for g in range(G):
            q = (pad[4 * g] + pad[4 * g + 1]) + (pad[4 * g + 2] + pad[4 * g + 3])
            acc[g % A] = q if g < A else acc[g % A] + q
        while len(acc) > 1:
            acc = [acc[2 * i] + acc[2 * i + 1] for i in range(len(acc) // 2)]
        assert acc[0].dtype == F32 and acc[0] == level_model(w, nfft), (nfft, K)


# ---- what the rule is for -------------------------------------------------------------------------------------------

ECHO_SHAPE = (2048, 1536, 5, 3, 1)  # mode I geometry, 5 symbols per frame: the FIC's three and one more


def echo_channel(nfft=2048):
    """two paths: H[k] = 1 + 0.9 e^j e^(-2 pi j 37 k / nfft), k the signed carrier number of the bin"""
    k = np.arange(nfft)
    k = np.where(k >= nfft // 2, k - nfft, k)
    return 1.0 + 0.9 * np.exp(1j) * np.exp(-2j * np.pi * 37 * k / nfft)


def echo_frames(O, snr_db, nframes=32, channel=True, seed=7):
    """-> (sent FIBs (4*nframes, 96), spectra (nframes, 5, 2048)): AWGN at snr_db relative to the first path"""
    rng = np.random.default_rng(seed)
    bins = freq_bins_model(2048)[1]
    fibs, tx = fic_bits(O, rng, nframes)
    bits = rng.integers(0, 2, (nframes, 4, 3072))
    bits[:, :3] = tx
    return fibs, transmit(bits, bins, ECHO_SHAPE, rng, carrier_gain=echo_channel() if channel else None, snr_db=snr_db)


def fib_errors(O, fibs, soft):
    """soft bytes (nframes, >= 3, 3072) -> (bit errors, FIBs of 32 bytes that differ from the ones sent)"""
    got = fic_decode(O, soft[:, :3].reshape(-1, 2304))
    diff = np.unpackbits(got ^ fibs, axis=1)
    return int(diff.sum()), int((got.reshape(-1, 32) != fibs.reshape(-1, 32)).any(axis=1).sum())


def test_the_echo_channel_costs_the_per_carrier_rule_its_fibs(O):
    """32 mode-I frames (384 FIBs) through the two-path channel at 4 dB: the per-carrier rule at its gain of 254 loses at
    least 50 FIBs, the per-symbol rule at gain 64 at most a quarter of that"""
    bins = freq_bins_model(2048)[1]
    fibs, z = echo_frames(O, 4.0)
    _, bad_carrier = fib_errors(O, fibs, demap_model(z, bins, ECHO_SHAPE, 254.0))
    _, bad_symbol = fib_errors(O, fibs, demap_soft_model(z, bins, ECHO_SHAPE, 64.0)[0])
    print("bad FIBs of 384: per carrier %d, per symbol %d" % (bad_carrier, bad_symbol))
    assert bad_carrier >= 50
    assert 4 * bad_symbol <= bad_carrier


# ---- the library without a GPU --------------------------------------------------------------------------------------

NEW_EXPORTS = ("vit_ofdm_demap_soft_dev", "vit_ofdm_demod_soft_dev")


def test_csi_exports(V):
    out = subprocess.check_output(["nm", "-D", "--defined-only", V.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in NEW_EXPORTS:
        assert name in exported and name in V.EXPORTS
        getattr(V.lib(), name)
    assert (V.SOFT_PER_CARRIER, V.SOFT_PER_SYMBOL) == (SOFT_PER_CARRIER, SOFT_PER_SYMBOL)
    assert C.sizeof(V.SoftRule) == 8 and V.SoftRule.gain.offset == 4


def test_csi_calls_fail_loudly(V):
    """without a device: VIT_ERR_NO_DEVICE before any argument is looked at, and an error text naming gfx950; with one,
    NULL buffers are VIT_ERR_ARG - nothing is launched either way.  The wrappers raise on arguments they can judge."""
    import torch
    want = 1 if torch.cuda.is_available() else 2  # VIT_ERR_ARG / VIT_ERR_NO_DEVICE
    L = V.lib()
    shape = V.OfdmShape(*MODE_I)
    for soft in (None, C.byref(V.SoftRule(SOFT_PER_SYMBOL, 64.0)), C.byref(V.SoftRule(7, 64.0))):
        assert L.vit_ofdm_demap_soft_dev(None, 2048, 76 * 2048, None, C.byref(shape), soft, 1, None, None, 0, None, None) == want
        if want == 2:
            assert "gfx950" in V.last_error()
        assert L.vit_ofdm_demod_soft_dev(None, None, None, C.byref(shape), soft, 1, None, None, 0, None, None) == want
        if want == 2:
            assert "gfx950" in V.last_error()
    host = torch.zeros(8, dtype=torch.float32)
    bins = torch.zeros(4, dtype=torch.int16)
    for bad_rule in (2, -1, None, 1.5):
        with pytest.raises(ValueError):
            V.ofdm_demap_soft_dev(host, MODE_I, bins, bad_rule, 64.0, 1)
        with pytest.raises(ValueError):
            V.ofdm_demod_soft_dev(host, MODE_I, bins, bad_rule, 64.0, 1, host, 2552, 196608)
    with pytest.raises(ValueError):
        V.ofdm_demap_soft_dev(host, MODE_I, bins, SOFT_PER_SYMBOL, 64.0, 1)  # tensors that are not on the device
    with pytest.raises(ValueError):
        V.ofdm_demod_soft_dev(host, MODE_I, bins, SOFT_PER_SYMBOL, 64.0, 1, host, 2552, 196608)
    with pytest.raises(ValueError):
        V.ofdm_demap_soft_dev(host, MODE_I, bins, SOFT_PER_SYMBOL, 64.0, 1, d_level=host)  # d_level on the host, and too short
    with pytest.raises(ValueError):
        V.ofdm_demod_soft_dev(host, MODE_I, bins, SOFT_PER_SYMBOL, 64.0, 1, host, 2552, d_level=None)  # no frame_stride


# ---- the table of INTEGRATION.md 2i ---------------------------------------------------------------------------------

def sensitivity_table(O, snrs=(3.0, 4.0, 5.0)):
    """rows (channel, snr_db, [(rule, gain, bit errors, bad FIBs)]) for the echo channel and, at the first SNR, a flat one"""
    bins = freq_bins_model(2048)[1]
    rows = []
    for channel, snr in [(True, s) for s in snrs] + [(False, snrs[0])]:
        fibs, z = echo_frames(O, snr, channel=channel)
        cells = [("per carrier", 254.0) + fib_errors(O, fibs, demap_model(z, bins, ECHO_SHAPE, 254.0))]
        for gain in (64.0, 128.0):
            cells.append(("per symbol", gain) + fib_errors(O, fibs, demap_soft_model(z, bins, ECHO_SHAPE, gain)[0]))
        rows.append(("echo" if channel else "flat", snr, cells))
    return rows


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import _vitpkg
    for channel, snr, cells in sensitivity_table(_vitpkg.load_oracle()):
        print("%s %g dB | " % (channel, snr) + " | ".join("%s, gain %g: %d bit errors, %d of 384 FIBs bad" % c for c in cells))
