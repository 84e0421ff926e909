"""GPU: vit_ofdm_demap_dev against the numpy float32 model of tests/test_ofdm_host.py - byte-exact, every output byte,
the guards and the poison around them included - and end to end into vit_decode_fic_dev and
vit_dabplus_ti_superframes_dev with no model in the loop."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (torch's runtime first, as when the whole suite is collected)

from test_gpu_dab import dabplus_superframes, decodable_segments
from test_dab_host import scramble
from test_ofdm_host import (MODE_I, MODE_II, MODE_III, MODE_IV, demap_model, fic_bits, freq_bins_model,
                            random_carrier_gain, special_carriers, split_model, transmit)
from test_punct_host import fic_segments, puncture
from test_ti_host import interleave

pytestmark = pytest.mark.gpu

GUARD = 64
FIC_GUARD = 0xEE
POISON = 0xA5
NAN = np.complex64(complex(np.nan, np.nan))


def ceil_div(a, b):
    return -(-a // b)


# The launch geometry of csrc/vit_ofdm.hip, mirrored: a workgroup owns one frame and a run of at most 25 consecutive
# data symbols, about 8 workgroups per CU over the grid; a CU holds at most 8 such workgroups (4 wavefronts each, 8
# wavefronts per SIMD).
def launch_geometry(torch, nframes, nsym):
    """-> (data symbols per run, workgroups of the grid, workgroups the device can hold at once at most)"""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    rpf = min(ceil_div(8 * cus, nframes), nsym)
    run = min(ceil_div(nsym, rpf), 25)
    return run, nframes * ceil_div(nsym, run), 8 * cus


def dev_bins(bins):
    return torch.from_numpy(np.ascontiguousarray(bins, np.uint16).view(np.int16)).cuda()


def nan_outside(z, bins):
    """NaN in every bin `bins` does not name: DC, the guard band, everything"""
    z = np.array(z, np.complex64)
    unused = np.ones(z.shape[-1], bool)
    unused[np.asarray(bins, np.int64)] = False
    z[..., unused] = NAN
    return z


def upload(z, shape, sym_stride, frame_stride):
    """(nframes, nsyms, nfft) complex64 -> device float32 pairs at the given strides, NaN in every gap; the buffer ends
    with the last symbol's last bin"""
    nfft, nsyms = shape[0], shape[2]
    nframes = z.shape[0]
    host = np.full((nframes - 1) * frame_stride + (nsyms - 1) * sym_stride + nfft, NAN, np.complex64)
    for t in range(nframes):
        for l in range(nsyms):
            o = t * frame_stride + l * sym_stride
            host[o:o + nfft] = z[t, l]
    return torch.from_numpy(host.view(np.float32)).cuda()


def run_case(V, z, bins, shape, gain, use_fic=True, use_ring=True, nrows=None, first_row=0, col=0, extra=0,
             sym_stride=None, frame_stride=None, fic_offset=3, ring_offset=1, d_bins=None, check=True):
    """one call on poisoned, guarded buffers at odd offsets; the whole buffers are compared with the model's image of
    them.  -> (fic buffer, ring buffer, expected fic buffer, expected ring buffer) as host arrays"""
    nfft, K, nsyms, fic_syms, cifs = shape
    nframes = z.shape[0]
    per = (nsyms - 1 - fic_syms) // cifs
    ss = nfft if sym_stride is None else sym_stride
    fs = nsyms * ss if frame_stride is None else frame_stride
    d_fft = upload(z, shape, ss, fs)
    nrows = nframes * cifs if nrows is None else nrows
    row_bytes = col + per * 2 * K + extra
    fic_n = nframes * fic_syms * 2 * K
    fic_buf = torch.full((fic_offset + fic_n + GUARD,), FIC_GUARD, dtype=torch.uint8, device="cuda")
    ring_buf = torch.full((ring_offset + nrows * row_bytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    d_ring = ring_buf[ring_offset:ring_offset + nrows * row_bytes].view(nrows, row_bytes)
    V.ofdm_demap_dev(d_fft, shape, dev_bins(bins) if d_bins is None else d_bins, gain, nframes,
                     d_fic=fic_buf[fic_offset:] if use_fic else None, d_ring=d_ring if use_ring else None,
                     first_row=first_row, col=col, sym_stride=ss, frame_stride=fs)
    torch.cuda.synchronize()
    want_fic = np.full(fic_buf.numel(), FIC_GUARD, np.uint8)
    want_ring = np.full(ring_buf.numel(), POISON, np.uint8)
    out = demap_model(z, bins, shape, gain)
    split_model(out, shape, fic=want_fic[fic_offset:fic_offset + fic_n] if use_fic else None,
                ring=want_ring[ring_offset:ring_offset + nrows * row_bytes].reshape(nrows, row_bytes) if use_ring else None,
                first_row=first_row, col=col)
    got_fic, got_ring = fic_buf.cpu().numpy(), ring_buf.cpu().numpy()
    if check:
        assert np.array_equal(got_fic, want_fic), "d_fic and its guards"
        assert np.array_equal(got_ring, want_ring), "the ring, its poison and its guards"
    return got_fic, got_ring, want_fic, want_ring


# ---- input families -------------------------------------------------------------------------------------------------

def family(name, rng, bins, shape, nframes):
    nfft, K, nsyms = shape[0], shape[1], shape[2]
    if name in ("tx30", "tx5"):
        bits = rng.integers(0, 2, (nframes, nsyms - 1, 2 * K))
        z = transmit(bits, bins, shape, rng, carrier_gain=random_carrier_gain(rng, nfft), snr_db=30.0 if name == "tx30" else 5.0)
    elif name in ("binades", "wide"):
        # uniform mantissas and signs over many binades: products over 2^-90 ... 2^90 (some below the 2^-64 bound), or for
        # "wide" over 2^-126 ... 2^126 (overflow to Inf, s = gain/nrm denormal)
        e = 45 if name == "binades" else 63
        mag = rng.uniform(1.0, 2.0, (nframes, nsyms, nfft, 2)) * 2.0 ** rng.integers(-e, e + 1, (nframes, nsyms, nfft, 2))
        v = (mag * rng.choice([-1.0, 1.0], mag.shape)).astype(np.float32)
        z = v.view(np.complex64)[..., 0]
    elif name == "special":
        bits = rng.integers(0, 2, (nframes, nsyms - 1, 2 * K))
        z = transmit(bits, bins, shape, rng)
        if K >= 6:
            for sym in range(0, nsyms, 3):
                special_carriers(z, bins, sym)
        else:
            z[:, nsyms // 2, bins[0]] = 0
    elif name == "ties":
        # b = a unit, a = (x + jy) b with x odd, |x| + |y| = 256: nrm = 256 and at gain 128 re*s = x/2, a tie
        x = (2 * rng.integers(0, 128, (nframes, nsyms, nfft)) + 1) * rng.choice([-1, 1], (nframes, nsyms, nfft))
        y = (256 - np.abs(x)) * rng.choice([-1, 1], x.shape)
        z = np.zeros((nframes, nsyms, nfft), np.complex128)
        unit = np.array([1, 1j, -1, -1j])
        for l in range(nsyms):  # even symbols are units, odd ones units times (x + jy)
            u = unit[rng.integers(0, 4, (nframes, nfft))]
            z[:, l] = u if l % 2 == 0 else u * (x[:, l] + 1j * y[:, l])
        z = z.astype(np.complex64)
    else:
        raise ValueError(name)
    return nan_outside(z, bins)


FAMILIES = ("tx30", "tx5", "binades", "wide", "special", "ties")


def subset_bins(rng, nfft, K):
    """a table that is not the standard's: a random permutation of a random subset of all bins, DC allowed"""
    return rng.permutation(nfft)[:K].astype(np.int64)


# nfft, K, nsyms, fic_syms, cifs; bins "std" or "rand"
ODD_SHAPES = [
    ((64, 1, 5, 1, 1), "rand"),        # K = 1: 2 bytes per symbol
    ((64, 7, 6, 2, 3), "rand"),        # K odd, 14 bytes per symbol (< 16), per = 1
    ((128, 77, 9, 0, 4), "rand"),      # K odd, no FIC symbols, per = 2
    ((256, 192, 12, 3, 8), "std"),     # per = 1
    ((1024, 1024, 4, 1, 1), "rand"),   # every bin is a carrier
    ((4096, 3001, 4, 1, 2), "rand"),   # the 1024-thread workgroups
    ((8192, 8192, 3, 1, 1), "rand"),
    ((2048, 1536, 4, 3, 1), "std"),    # nsyms - 1 = fic_syms: a frame has no CIF
]


@pytest.mark.parametrize("shape", [MODE_I, MODE_II, MODE_III, MODE_IV])
@pytest.mark.parametrize("fam", FAMILIES)
def test_modes_against_the_model(V, torch_cuda, shape, fam):
    """the four transmission modes with the standard's table, every input family, nframes 1 and 3, d_fic and ring, a ring
    whose call rows wrap, odd col / row_bytes / buffer offsets, NaN in every bin the table does not name"""
    rng = np.random.default_rng(10 * shape[0] + FAMILIES.index(fam))
    bins = freq_bins_model(shape[0])[1]
    gain = 128.0 if fam == "ties" else 254.0
    for nframes in (1, 3):
        z = family(fam, rng, bins, shape, nframes)
        nrows = nframes * shape[4] + 15 + 2
        run_case(V, z, bins, shape, gain, nrows=nrows, first_row=nrows - 2, col=7, extra=4)


@pytest.mark.parametrize("shape,kind", ODD_SHAPES)
def test_odd_shapes_against_the_model(V, torch_cuda, shape, kind):
    """K = 1, odd K, tables that are not the standard's, per = 1, no FIC symbols, no CIFs, the largest FFT lengths; strides
    with gaps full of NaN; d_fic only, ring only, both"""
    rng = np.random.default_rng(shape[0] + shape[1])
    nfft, K, nsyms, fic_syms, cifs = shape
    bins = freq_bins_model(nfft)[1] if kind == "std" else subset_bins(rng, nfft, K)
    for fam in ("tx5", "binades", "special", "ties"):
        gain = 128.0 if fam == "ties" else float(rng.choice([1.0, 127.0, 180.5, 254.0, 65536.0]))
        for nframes, use_fic, use_ring in ((1, True, True), (4, True, False), (5, False, True), (2, True, True)):
            z = family(fam, rng, bins, shape, nframes)
            ss = nfft + 2 * int(rng.integers(0, 9))
            fs = nsyms * ss + 2 * int(rng.integers(0, 50))
            nrows = nframes * cifs + int(rng.integers(0, 20))
            run_case(V, z, bins, shape, gain, use_fic=use_fic, use_ring=use_ring, nrows=nrows,
                     first_row=int(rng.integers(0, nrows)), col=int(rng.integers(0, 40)), extra=int(rng.integers(1, 9)),
                     sym_stride=ss, frame_stride=fs, fic_offset=int(rng.integers(0, 8)), ring_offset=int(rng.integers(0, 8)))


def test_unnamed_bins_influence_nothing(V, torch_cuda):
    """the same carriers with zeros, with NaN and with random numbers in DC, the guard band and every other unnamed bin"""
    rng = np.random.default_rng(11)
    shape = MODE_IV
    bins = freq_bins_model(1024)[1]
    bits = rng.integers(0, 2, (2, 75, 2 * 768))
    z0 = transmit(bits, bins, shape, rng, snr_db=8.0)
    unused = np.ones(1024, bool)
    unused[bins] = False
    outs = []
    for fill in ("zero", "nan", "rand"):
        z = z0.copy()
        if fill == "nan":
            z[..., unused] = NAN
        elif fill == "rand":
            z[..., unused] = (rng.standard_normal((2, 76, int(unused.sum()))) * 1e30).astype(np.complex64)
        outs.append(run_case(V, z, bins, shape, 200.0, col=1, extra=1)[:2])
    for f, r in outs[1:]:
        assert np.array_equal(f, outs[0][0]) and np.array_equal(r, outs[0][1])


def test_first_row_carried_over_two_calls(V, torch_cuda):
    """a streaming ring: 3 frames into rows r0 ..., then 2 frames into the rows after them (wrapping); rows of neither call
    - the de-interleaver's overlap among them - keep their poison"""
    torch = torch_cuda
    rng = np.random.default_rng(12)
    shape = MODE_II  # 1 CIF per frame, per*2K = 55296
    nfft, K, nsyms, fic_syms, cifs = shape
    bins = freq_bins_model(nfft)[1]
    z = family("tx5", rng, bins, shape, 5)
    nrows, row_bytes, col = 5 + 15, 55296 + 3, 3
    d_fft = upload(z, shape, nfft, nsyms * nfft)
    d_b = dev_bins(bins)
    buf = torch.full((1 + nrows * row_bytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    d_ring = buf[1:1 + nrows * row_bytes].view(nrows, row_bytes)
    d_fic = torch.full((5 * 3 * 2 * K + GUARD,), FIC_GUARD, dtype=torch.uint8, device="cuda")
    r0 = nrows - 4
    V.ofdm_demap_dev(d_fft, shape, d_b, 254.0, 3, d_fic=d_fic, d_ring=d_ring, first_row=r0, col=col)
    r1 = (r0 + 3 * cifs) % nrows
    V.ofdm_demap_dev(d_fft[3 * nsyms * nfft * 2:], shape, d_b, 254.0, 2, d_fic=d_fic[3 * 3 * 2 * K:], d_ring=d_ring, first_row=r1,
                     col=col)
    torch.cuda.synchronize()
    want = np.full(buf.numel(), POISON, np.uint8)
    want_fic = np.full(d_fic.numel(), FIC_GUARD, np.uint8)
    out = demap_model(z, bins, shape, 254.0)
    split_model(out, shape, fic=want_fic[:5 * 3 * 2 * K], ring=want[1:1 + nrows * row_bytes].reshape(nrows, row_bytes),
                first_row=r0, col=col)
    assert np.array_equal(buf.cpu().numpy(), want) and np.array_equal(d_fic.cpu().numpy(), want_fic)
    touched = {(r0 + i) % nrows for i in range(5)}
    ring = buf.cpu().numpy()[1:1 + nrows * row_bytes].reshape(nrows, row_bytes)
    assert all((ring[r] == POISON).all() for r in range(nrows) if r not in touched)


def test_large_batch(V, torch_cuda):
    """2304 mode-I frames in one call (2.9 GB in), 256 distinct frames tiled on the device: every workgroup's run is 25
    symbols long and the grid is three times what the device holds at once; compared per distinct frame"""
    torch = torch_cuda
    shape = MODE_I
    nfft, K, nsyms, fic_syms, cifs = shape
    base_n, reps = 256, 9
    nframes = base_n * reps
    assert nframes >= 2048
    run, grid, resident = launch_geometry(torch, nframes, nsyms - 1)
    assert run >= 16 and grid >= 3 * resident, (run, grid, resident)
    rng = np.random.default_rng(13)
    bins = freq_bins_model(nfft)[1]
    v = (rng.standard_normal((base_n, nsyms, nfft, 2), dtype=np.float32) *
         (2.0 ** rng.integers(-8, 9, (base_n, nsyms, nfft, 1))).astype(np.float32))
    z = nan_outside(v.view(np.complex64)[..., 0], bins)
    want = np.concatenate([demap_model(z[i:i + 32], bins, shape, 254.0) for i in range(0, base_n, 32)])  # (256, 75, 3072)
    d_base = torch.from_numpy(z.view(np.float32).reshape(base_n, -1)).cuda()
    d_fft = d_base.repeat(reps, 1).contiguous()
    del d_base
    nrows, col, row_bytes = nframes * cifs + 15 + 6, 5, 5 + 55296 + 2
    first_row = nrows - 1000
    ring_buf = torch.full((1 + nrows * row_bytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    d_ring = ring_buf[1:1 + nrows * row_bytes].view(nrows, row_bytes)
    fic_n = nframes * 9216
    fic_buf = torch.full((3 + fic_n + GUARD,), FIC_GUARD, dtype=torch.uint8, device="cuda")
    V.ofdm_demap_dev(d_fft, shape, dev_bins(bins), 254.0, nframes, d_fic=fic_buf[3:], d_ring=d_ring, first_row=first_row, col=col)
    torch.cuda.synchronize()
    del d_fft
    d_want = torch.from_numpy(want).cuda()
    assert bool((fic_buf[:3] == FIC_GUARD).all()) and bool((fic_buf[3 + fic_n:] == FIC_GUARD).all())
    assert bool((fic_buf[3:3 + fic_n].view(reps, base_n, 9216) == d_want[:, :3].reshape(1, base_n, 9216)).all())
    assert bool((ring_buf[:1] == POISON).all()) and bool((ring_buf[1 + nrows * row_bytes:] == POISON).all())
    assert bool((d_ring[:, :col] == POISON).all()) and bool((d_ring[:, col + 55296:] == POISON).all())
    rows = (first_row + torch.arange(nframes * cifs, device="cuda")) % nrows
    want_rows = d_want[:, 3:].reshape(1, base_n * cifs, 55296)
    for r in range(reps):  # one repetition's rows at a time
        got = d_ring[rows[r * base_n * cifs:(r + 1) * base_n * cifs], col:col + 55296]
        assert bool((got == want_rows[0]).all()), r
    other = torch.ones(nrows, dtype=torch.bool, device="cuda")
    other[rows] = False
    assert int(other.sum()) == 21 and bool((d_ring[other] == POISON).all())


# ---- arguments ------------------------------------------------------------------------------------------------------

def test_argument_errors(V, torch_cuda):
    """every rule is VIT_ERR_ARG with a message and launches nothing; an empty batch is VIT_OK and writes nothing"""
    torch = torch_cuda
    L = V.lib()
    shape = MODE_II
    nfft, K, nsyms = 512, 384, 76
    d_fft = torch.zeros(2 * (2 * nsyms * nfft) + 8, dtype=torch.float32, device="cuda")
    d_b = dev_bins(freq_bins_model(nfft)[1])
    d_fic = torch.full((2 * 3 * 2 * K,), 0x33, dtype=torch.uint8, device="cuda")
    d_ring = torch.full((4, 55296 + 10), 0x33, dtype=torch.uint8, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fft, bins, fic = C.c_void_p(d_fft.data_ptr()), C.c_void_p(d_b.data_ptr()), C.c_void_p(d_fic.data_ptr())

    def ring(**kw):
        r = V.cif_ring(d_ring, 0)
        for k, v in kw.items():
            setattr(r, k, v)
        return C.byref(r)

    def call(fft=fft, ss=nfft, fs=nsyms * nfft, bins=bins, shape=shape, gain=254.0, nframes=2, fic=fic, ring=ring(), col=0):
        sh = None if shape is None else C.byref(V.OfdmShape(*shape))
        return L.vit_ofdm_demap_dev(fft, ss, fs, bins, sh, gain, nframes, fic, ring, col, s)

    bad = [dict(fft=None), dict(bins=None), dict(shape=None), dict(fic=None, ring=None), dict(nframes=-1),
           dict(fft=C.c_void_p(d_fft.data_ptr() + 8)), dict(fft=C.c_void_p(d_fft.data_ptr() + 4)), dict(ss=nfft + 1),
           dict(fs=nsyms * nfft + 1), dict(ss=nfft - 2),
           dict(shape=(500, 384, 76, 3, 1)), dict(shape=(32, 24, 76, 3, 1)), dict(shape=(16384, 384, 76, 3, 1)),
           dict(shape=(512, 0, 76, 3, 1)), dict(shape=(512, 513, 76, 3, 1)), dict(shape=(512, 384, 3, 3, 1)),
           dict(shape=(512, 384, 76, 3, 0)), dict(shape=(512, 384, 76, 3, 5)), dict(shape=(512, 384, 0, 0, 1)),
           dict(gain=0.0), dict(gain=-1.0), dict(gain=65537.0), dict(gain=float("inf")), dict(gain=float("nan")),
           dict(ring=ring(d_base=None)), dict(ring=ring(first_row=4)), dict(ring=ring(first_row=5)),
           dict(nframes=5), dict(ring=ring(nrows=1)), dict(col=11), dict(ring=ring(row_bytes=55295)),
           dict(col=(1 << 64) - 1)]
    for kw in bad:
        assert call(**kw) == 1, kw
        assert "bad arguments" in V.last_error(), kw
    assert call(nframes=0) == 0
    torch.cuda.synchronize()
    assert bool((d_fic == 0x33).all()) and bool((d_ring == 0x33).all())
    assert call() == 0 and call(col=10) == 0 and call(fic=None) == 0 and call(ring=None) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        V.ofdm_demap_dev(d_fft.to(torch.float64), shape, d_b, 254.0, 1, d_fic=d_fic)
    with pytest.raises(ValueError):
        V.ofdm_demap_dev(d_fft, shape, d_b.to(torch.int32), 254.0, 1, d_fic=d_fic)


def test_bad_bins_tables_stay_inside_the_call_s_bytes(V, torch_cuda):
    """entries >= nfft and repeated entries: the bytes of the carriers involved are unspecified, every other carrier's
    bytes are the model's, and guards and poison survive"""
    rng = np.random.default_rng(14)
    shape = MODE_III
    nfft, K, nsyms, fic_syms, cifs = shape
    bins = freq_bins_model(nfft)[1].copy()
    z = family("tx5", rng, bins, shape, 2)
    broken = bins.copy()
    big = rng.choice(K, 20, replace=False)
    broken[big[:10]] = rng.integers(nfft, 65536, 10)
    broken[big[:3]] = [nfft, 65535, 32768]
    broken[big[10:]] = bins[(big[10:] + 7) % K]  # repeats of entries that stay in the table
    involved = np.zeros(K, bool)
    involved[big] = True
    involved[(big[10:] + 7) % K] = True
    got_fic, got_ring, want_fic, want_ring = run_case(V, z, bins, shape, 254.0, nrows=2 + 3, first_row=4, col=3, extra=5,
                                                      d_bins=dev_bins(broken), check=False)
    # which bytes of the expected images belong to involved carriers: run the model's split on a marker
    mark = np.zeros((2, nsyms - 1, 2 * K), np.uint8)
    mark[:, :, np.concatenate([involved, involved])] = 1
    m_fic, m_ring = np.zeros_like(want_fic), np.zeros_like(want_ring)
    per = (nsyms - 1 - fic_syms) // cifs
    row_bytes = 3 + per * 2 * K + 5
    split_model(mark, shape, fic=m_fic[3:3 + 2 * fic_syms * 2 * K], ring=m_ring[1:1 + 5 * row_bytes].reshape(5, row_bytes),
                first_row=4, col=3)
    assert m_fic.sum() + m_ring.sum() == mark.sum()
    assert np.array_equal(got_fic[m_fic == 0], want_fic[m_fic == 0])
    assert np.array_equal(got_ring[m_ring == 0], want_ring[m_ring == 0])


# ---- end to end -----------------------------------------------------------------------------------------------------

def test_end_to_end_fic_and_dabplus(V, O, torch_cuda):
    """no model in the loop: 10 mode-I frames carrying 40 FIC coding blocks (120 FIBs) and, in their 40 CIFs, 5 DAB+
    superframes of one time-interleaved sub-channel, through a frequency-selective channel with AWGN (11 dB carrier SNR) ->
    vit_ofdm_demap_dev -> vit_decode_fic_dev on d_fic and vit_dabplus_ti_superframes_dev on the ring"""
    torch = torch_cuda
    rng = np.random.default_rng(15)
    shape = MODE_I
    nfft, K, nsyms, fic_syms, cifs = shape
    nframes, nsf, rsdims, start_cu = 10, 5, 24, 3
    fb = 192 * rsdims
    bins = freq_bins_model(nfft)[1]
    fibs, fic_tx = fic_bits(O, rng, nframes)
    pay, sf = dabplus_superframes(rng, nsf, rsdims)
    frames = scramble(sf.reshape(-1, 24 * rsdims), fb)
    coded = np.stack([O.encode(b) for b in np.unpackbits(frames, axis=1)]).astype(np.uint8)
    segs = decodable_segments(rng, fb)
    punct = puncture(coded, segs, fb)
    P = punct.shape[1]
    cif = rng.integers(0, 2, (5 * nsf + 15, 55296), dtype=np.uint8)
    assert cif.shape[0] == nframes * cifs and 64 * start_cu + P <= 55296
    cif[:, 64 * start_cu:64 * start_cu + P] = interleave(punct)
    bits = np.zeros((nframes, nsyms - 1, 2 * K), np.int64)
    bits[:, :fic_syms] = fic_tx
    bits[:, fic_syms:] = cif.reshape(nframes, nsyms - 1 - fic_syms, 2 * K)
    z = nan_outside(transmit(bits, bins, shape, rng, carrier_gain=random_carrier_gain(rng, nfft), snr_db=11.0), bins)
    d_fft = torch.from_numpy(z.view(np.float32)).cuda()
    nrows, first_row, col = 44, 41, 9
    d_ring = torch.full((nrows, col + 55296 + 1), POISON, dtype=torch.uint8, device="cuda")
    d_fic = torch.full((nframes * 9216,), FIC_GUARD, dtype=torch.uint8, device="cuda")
    V.ofdm_demap_dev(d_fft, shape, dev_bins(bins), 180.0, nframes, d_fic=d_fic, d_ring=d_ring, first_row=first_row, col=col)
    nblk = 4 * nframes
    d_fibs = torch.zeros((nblk, 96), dtype=torch.uint8, device="cuda")
    d_ok = torch.zeros((nblk * 3,), dtype=torch.uint8, device="cuda")
    V.decode_fic_dev(d_fic, d_fibs, d_ok, 768, nblk, fic_segments())
    d_work = torch.zeros((nsf, 120 * rsdims), dtype=torch.uint8, device="cuda")
    d_out = torch.zeros((nsf, 110 * rsdims), dtype=torch.uint8, device="cuda")
    d_ret = torch.full((nsf,), -7, dtype=torch.int32, device="cuda")
    d_fire = torch.zeros((nsf,), dtype=torch.uint8, device="cuda")
    V.dabplus_ti_superframes_dev(d_ring, first_row, col + 64 * start_cu, segs, d_work, d_out, d_ret, rsdims, nsf, d_fire_ok=d_fire)
    torch.cuda.synchronize()
    assert bool((d_ok == 1).all())
    assert np.array_equal(d_fibs.cpu().numpy(), fibs)
    assert bool((d_fire == 1).all()) and bool((d_ret >= 0).all())
    assert np.array_equal(d_out.cpu().numpy(), pay)
