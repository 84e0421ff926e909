"""CPU-only: "From the samples" (include/viterbi_amd.h) - the definition of the front end as a numpy float32 model
independent of the library (rotate_model, fft_model: one float32 ufunc per operation, vectorised per stage), pinned by
its accuracy against a float64 FFT, the two host tables against their definition, and a time-domain transmitter (the
model transmitter of tests/test_ofdm_host.py -> inverse FFT -> cyclic prefix) whose bits the models recover.
tests/test_gpu_ofdm_td.py uses the same models as its exact reference."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from test_ofdm_host import MODE_I, MODE_II, MODE_III, demap_model, freq_bins_model, transmit

F32 = np.float32
LENGTHS = (64, 128, 256, 512, 1024, 2048, 4096, 8192)
U = 2.0 ** -24  # unit roundoff of binary32


# ---- the definition -------------------------------------------------------------------------------------------------

def unit_table(n, sign):
    """(cos, sign*sin)(2 pi k / n), k < n: binary64 rounded to binary32, exact at multiples of an eighth of a turn"""
    k = np.arange(n)
    a = 2.0 * np.pi * k / n
    t = np.stack([np.cos(a), sign * np.sin(a)], axis=1).astype(F32)
    if n >= 8:
        r = F32(np.sqrt(0.5))
        c = np.array([1, r, 0, -r, -1, -r, 0, r], F32)
        s = np.array([0, r, 1, r, 0, -r, -1, -r], F32)
        t[::n // 8, 0] = c
        t[::n // 8, 1] = F32(sign) * s
    else:
        t[:] = {1: [[1, 0]], 2: [[1, 0], [-1, 0]], 4: [[1, 0], [0, sign], [-1, 0], [0, -sign]]}[n]
    return t + F32(0)  # -0 -> +0


def twiddles_model(nfft):
    return unit_table(nfft, -1.0)[:nfft // 2]


def nco_model(bits):
    return unit_table(1 << bits, 1.0)


def bitrev_perm(m):
    i = np.arange(1 << m)
    r = np.zeros_like(i)
    for b in range(m):
        r |= (i >> b & 1) << (m - 1 - b)
    return r


def cmul_model(ar, ai, br, bi):
    """fl(fl(ar*br) - fl(ai*bi)), fl(fl(ar*bi) + fl(ai*br)) on float32 arrays"""
    assert ar.dtype == F32 and ai.dtype == F32 and br.dtype == F32 and bi.dtype == F32
    return ar * br - ai * bi, ar * bi + ai * br


def fft_model(x, tw):
    """x: (..., nfft) complex64, tw: (nfft/2, 2) float32 -> (..., nfft) complex64: the header's radix-2 decimation in time,
    every operation one numpy float32 operation"""
    x = np.asarray(x, np.complex64)
    nfft = x.shape[-1]
    m = nfft.bit_length() - 1
    assert nfft == 1 << m and tw.shape == (nfft // 2, 2) and tw.dtype == F32
    lead = x.shape[:-1]
    perm = bitrev_perm(m)
    re = np.ascontiguousarray(x.real[..., perm]).reshape(-1, nfft)
    im = np.ascontiguousarray(x.imag[..., perm]).reshape(-1, nfft)
    with np.errstate(all="ignore"):
        for s in range(1, m + 1):
            h = 1 << (s - 1)
            w = tw[np.arange(h) * (nfft >> s)]
            re = re.reshape(-1, nfft >> s, 2, h)
            im = im.reshape(-1, nfft >> s, 2, h)
            ur, ui, vr, vi = re[:, :, 0], im[:, :, 0], re[:, :, 1], im[:, :, 1]
            tr, ti = cmul_model(np.broadcast_to(w[:, 0], vr.shape), np.broadcast_to(w[:, 1], vr.shape), vr, vi)
            re = np.stack([ur + tr, ur - tr], axis=2)
            im = np.stack([ui + ti, ui - ti], axis=2)
            assert re.dtype == F32
    out = np.empty((re.shape[0], nfft), np.complex64)
    out.real = re.reshape(-1, nfft)
    out.imag = im.reshape(-1, nfft)
    return out.reshape(lead + (nfft,))


def rotate_model(x, nco, nco_bits, rot, sym_stride):
    """x: (nframes, nsyms, nfft) complex64 useful parts; rot: (nframes, 2) of phase0, step; sample i of symbol l is sample
    n = l*sym_stride + i of its frame and is multiplied by nco[((phase0 + n*step) mod 2^32) >> (32 - nco_bits)]"""
    x = np.asarray(x, np.complex64)
    nframes, nsyms, nfft = x.shape
    rot = np.asarray(rot, np.uint64).reshape(nframes, 2)
    n = (np.arange(nsyms, dtype=np.uint64)[:, None] * np.uint64(sym_stride) + np.arange(nfft, dtype=np.uint64)[None, :])
    n = n & np.uint64(0xFFFFFFFF)
    ph = (rot[:, 0, None, None] + n[None] * rot[:, 1, None, None]) & np.uint64(0xFFFFFFFF)  # < 2^64: both factors < 2^32
    w = nco[(ph >> np.uint64(32 - nco_bits)).astype(np.int64)]
    with np.errstate(all="ignore"):
        re, im = cmul_model(np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag), w[..., 0], w[..., 1])
    out = np.empty(x.shape, np.complex64)
    out.real, out.imag = re, im
    return out


def front_model(x, tw, nco=None, nco_bits=0, rot=None, sym_stride=None):
    return fft_model(x if rot is None else rotate_model(x, nco, nco_bits, rot, sym_stride), tw)


# ---- the time-domain transmitter ------------------------------------------------------------------------------------

def time_domain(z, guard, cfo=0.0):
    """(nframes, nsyms, nfft) spectra -> (nframes, nsyms*(guard + nfft)) complex128 samples: inverse FFT (scaled to unit
    carriers), cyclic prefix of `guard` samples (any length) in front of every symbol, then a frequency offset of `cfo`
    carrier spacings, continuous over the frame"""
    nframes, nsyms, nfft = z.shape
    x = np.fft.ifft(np.asarray(z, np.complex128), axis=-1) * nfft
    x = x[..., np.arange(-guard, nfft) % nfft].reshape(nframes, -1)  # a guard longer than the symbol wraps around it
    n = np.arange(x.shape[1])
    return x * np.exp(2j * np.pi * cfo * n / nfft)[None, :]


def cfo_step(cfo, nfft):
    """the rotation that takes a frequency offset of `cfo` carrier spacings away: step = round(-df/fs 2^32) mod 2^32"""
    return int(round(-cfo / nfft * 2.0 ** 32)) % (1 << 32)


def useful_parts(x, start, shape, sym_stride):
    """x: one frame's samples -> (nsyms, nfft) complex64 windows from sample `start`"""
    nfft, nsyms = shape[0], shape[2]
    return np.stack([x[start + l * sym_stride:start + l * sym_stride + nfft] for l in range(nsyms)]).astype(np.complex64)


# ---- the model's accuracy -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nfft", LENGTHS)
def test_model_against_float64_fft(nfft):
    """relative L2 error <= 8 m u: Higham, Accuracy and Stability of Numerical Algorithms, Thm 24.2 bounds the radix-2 FFT
    with twiddles of relative error u by about 6.7 m u; the rest covers the tables' own rounding"""
    m = nfft.bit_length() - 1
    rng = np.random.default_rng(nfft)
    tw = twiddles_model(nfft)
    gauss = (rng.standard_normal((4, nfft)) + 1j * rng.standard_normal((4, nfft))).astype(np.complex64)
    k = np.array([0, 1, 3, nfft // 8, nfft // 4 + 1, nfft // 2, nfft - 1])
    tones = np.exp(2j * np.pi * k[:, None] * np.arange(nfft)[None, :] / nfft).astype(np.complex64)
    for x in (gauss, tones):
        got = fft_model(x, tw).astype(np.complex128)
        want = np.fft.fft(x.astype(np.complex128), axis=-1)
        err = np.linalg.norm(got - want, axis=-1) / np.linalg.norm(want, axis=-1)
        print("nfft %d: relative L2 error %.2f ... %.2f u" % (nfft, err.min() / U, err.max() / U))
        assert err.max() <= 8 * m * U
    assert np.abs(fft_model(tones, tw)[np.arange(k.size), k]).min() > 0.999 * nfft  # a tone lands in its bin


def test_model_skips_nothing_it_may_not():
    """the exact twiddles: multiplying by 1 and -j is the identity and a swap for every finite value, so an implementation
    that skips those products computes the same values (the header's domain)"""
    tw = twiddles_model(64)
    assert tw[0].tolist() == [1.0, 0.0] and tw[16].tolist() == [0.0, -1.0]
    v = np.array([3.25, -1e-30, 7e20, 0.0], F32)
    tr, ti = cmul_model(np.full(4, tw[16, 0]), np.full(4, tw[16, 1]), v, v[::-1].copy())
    assert np.array_equal(tr, v[::-1]) and np.array_equal(ti, -v)


# ---- the tables -----------------------------------------------------------------------------------------------------

def ulp_apart(a, b):
    """distance in float32 ulps, by value (-0 = +0)"""
    ia = np.asarray(a, F32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, F32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def check_table(got, want, n):
    assert got.dtype == F32 and got.shape == want.shape
    eighth = np.arange(got.shape[0]) % max(n // 8, 1) == 0
    assert np.array_equal(got[eighth], want[eighth])  # exact: 0, +-1, +-fl(sqrt 1/2)
    r = float(F32(np.sqrt(0.5)))
    assert set(np.abs(got[eighth]).ravel().tolist()) <= {0.0, 1.0, r}
    assert ulp_apart(got, want).max() <= 1  # two math libraries need not round identically


@pytest.mark.parametrize("nfft", LENGTHS)
def test_fft_twiddles(V, nfft):
    check_table(V.fft_twiddles(nfft), twiddles_model(nfft), nfft)


@pytest.mark.parametrize("bits", [1, 2, 3, 4, 10, 17, 20])
def test_nco_table(V, bits):
    check_table(V.nco_table(bits), nco_model(bits), 1 << bits)


def test_tables_return_values_and_rejections(V):
    L = V.lib()
    buf = np.full(2 * 4096 + 2, 7.5, F32)
    p = buf.ctypes.data_as(C.c_void_p)
    for nfft in LENGTHS:
        assert L.vit_fft_twiddles(nfft, p) == nfft // 2
        assert (buf[nfft:] == 7.5).all()
    buf[:] = 7.5
    for nfft in (0, 1, 2, 32, 63, 65, 100, 2047, 16384, 0x80000000, 0xFFFFFFFF):
        assert L.vit_fft_twiddles(nfft, p) == -1, nfft
        with pytest.raises(ValueError):
            V.fft_twiddles(nfft)
    assert L.vit_fft_twiddles(2048, None) == -1
    for bits in (1, 5, 12):
        assert L.vit_nco_table(bits, p) == 1 << bits
        assert (buf[2 << bits:] == 7.5).all()
        buf[:] = 7.5
    for bits in (0, 21, 32, 0xFFFFFFFF):
        assert L.vit_nco_table(bits, p) == -1, bits
        with pytest.raises(ValueError):
            V.nco_table(bits)
    assert L.vit_nco_table(8, None) == -1
    assert (buf == 7.5).all()


# ---- the transmitter through the models -----------------------------------------------------------------------------

@pytest.mark.parametrize("shape,guard", [(MODE_III, 63), (MODE_II, 126)])
def test_time_domain_transmitter_without_noise(shape, guard):
    """no noise, a start anywhere inside the guard: demap_model(fft_model(...)) makes the decisions of the transmitted bits"""
    nfft, K, nsyms = shape[0], shape[1], shape[2]
    rng = np.random.default_rng(30 + nfft)
    bins = freq_bins_model(nfft)[1]
    bits = rng.integers(0, 2, (2, nsyms - 1, 2 * K))
    x = time_domain(transmit(bits, bins, shape, rng), guard)
    tw = twiddles_model(nfft)
    ss = nfft + guard
    for start in (0, 1, guard // 2, guard - 1, guard):
        parts = np.stack([useful_parts(x[t], start, shape, ss) for t in range(2)])
        out = demap_model(fft_model(parts, tw), bins, shape, 254.0)
        assert np.array_equal(out > 128, bits.astype(bool)), start


def test_frequency_offset_needs_the_rotation():
    """0.3 carrier spacings of frequency offset: the decisions are right with the rotation and wrong without it"""
    shape, guard = MODE_III, 63
    nfft, K, nsyms = shape[0], shape[1], shape[2]
    rng = np.random.default_rng(40)
    bins = freq_bins_model(nfft)[1]
    bits = rng.integers(0, 2, (2, nsyms - 1, 2 * K))
    x = time_domain(transmit(bits, bins, shape, rng), guard, cfo=0.3)
    tw, ss = twiddles_model(nfft), nfft + guard
    parts = np.stack([useful_parts(x[t], guard // 2, shape, ss) for t in range(2)])
    plain = demap_model(fft_model(parts, tw), bins, shape, 254.0)
    assert not np.array_equal(plain > 128, bits.astype(bool))
    assert np.mean((plain > 128) != bits.astype(bool)) > 0.1
    for nco_bits in (10, 16, 20):
        rot = [[12345, cfo_step(0.3, nfft)], [0xF0000000, cfo_step(0.3, nfft)]]
        z = front_model(parts, tw, nco_model(nco_bits), nco_bits, rot, ss)
        assert np.array_equal(demap_model(z, bins, shape, 254.0) > 128, bits.astype(bool)), nco_bits


def test_rotate_model_wraps_the_phase():
    """step 2^31 alternates the sign, 2^32 - 1 runs backwards, the phase is taken mod 2^32, and the guards count"""
    x = np.ones((1, 2, 64), np.complex64)
    nco = nco_model(1)  # {1, -1}
    out = rotate_model(x, nco, 1, [[0, 1 << 31]], 65)
    assert np.array_equal(out[0, 0].real, np.where(np.arange(64) % 2 == 0, 1, -1))
    assert np.array_equal(out[0, 1].real, np.where((65 + np.arange(64)) % 2 == 0, 1, -1))
    nco = nco_model(20)
    out = rotate_model(x, nco, 20, [[5 << 12, (1 << 32) - (1 << 12)]], 64)
    idx = (5 - np.arange(128)) % (1 << 20)
    assert np.array_equal(out.reshape(-1).view(F32).reshape(-1, 2), nco[idx])


# ---- the library without a GPU --------------------------------------------------------------------------------------

NEW_EXPORTS = ("vit_fft_twiddles", "vit_nco_table", "vit_ofdm_fft_dev", "vit_ofdm_demod_dev")


def test_ofdm_td_exports(V):
    out = subprocess.check_output(["nm", "-D", "--defined-only", V.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in NEW_EXPORTS:
        assert name in exported and name in V.EXPORTS


def test_ofdm_td_calls_fail_loudly(V):
    """without a device: VIT_ERR_NO_DEVICE and an error text naming gfx950; with one, NULL buffers are VIT_ERR_ARG -
    nothing is launched either way; the host helpers work without one"""
    import torch
    want = 1 if torch.cuda.is_available() else 2  # VIT_ERR_ARG / VIT_ERR_NO_DEVICE
    shape = V.OfdmShape(*MODE_I)
    inp = V.IqInput()
    inp.sym_stride, inp.frame_stride = 2552, 196608
    assert V.lib().vit_ofdm_demod_dev(C.byref(inp), None, C.byref(shape), 254.0, 1, None, None, 0, None) == want
    if want == 2:
        assert "gfx950" in V.last_error()
    assert V.lib().vit_ofdm_fft_dev(C.byref(inp), 2048, 76, 1, None, 2048, 76 * 2048, None) == want
    if want == 2:
        assert "gfx950" in V.last_error()
    assert C.sizeof(V.IqInput) == 72 and V.IqInput.nco_bits.offset == 56 and V.IqInput.d_rot.offset == 64
    assert V.fft_twiddles(64).shape == (32, 2) and V.nco_table(3).shape == (8, 2)
