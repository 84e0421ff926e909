"""GPU: "Before the stream: rate conversion and channel selection" - vit_iq_resample_dev against the numpy float32 model
of tests/test_resample_host.py in every output word.  Every call goes through the C ABI; the output buffer is filled with
a sentinel and compared whole with the model's image, so a write outside the named elements - the gaps between channels
when out_stride > nout among them - fails; the device's samples are poisoned (NaN, or the codes' complements) wherever no
requested output needs them - in front of the first needed sample, behind the last one, in the gaps of a ratio with
M > L*T - so a read of what must not be read fails too.  The shapes are those at which the kernel takes another path: each
tile size around its edge, several tiles, one workgroup's span at its cap, threads that read their samples from memory,
P beyond 2^32, the four sample formats at their least alignment, 1 to 16 channels with and without rotation."""
import numpy as np
import pytest
import torch  # noqa: F401  (torch's runtime first, as when the whole suite is collected)

from test_acq_host import acquire_model
from test_fft_host import F32
from test_gpu_iqfmt import dev_raw
from test_gpu_ofdm import dev_bins
from test_gpu_ofdm_td import dev_u32, nco_tables, tw_tables
from test_iqfmt_host import INT_FORMATS, IQ_CS16, IQ_CU8, convert_model, quantise
from test_ofdm_host import MODE_I
from test_resample_host import (CHAIN_FRAMES, Rs, chain_case, chain_params, continuation, out_count_model, random_taps,
                                replay_argument_errors, resample_model)

pytestmark = pytest.mark.gpu

IQ_F32 = 0
FORMATS = (IQ_F32,) + INT_FORMATS
SENT = np.array([0x5A5A5A5A], np.uint32).view(F32)[0]  # a finite float no output equals
GW = 5  # guard elements around the output image
# (L, M, T, pos0): the identity ratio; decimation by 2; upsampling, where n0 repeats; the two production shapes, the second
# with L*T at its cap; a start in mid-phase past sample 0 (for CU8: a first needed sample at an address that is 2 mod 4); a
# workgroup's span at its cap (tile 16); M > L*T twice: threads read their own samples, gaps in between
SHAPES = [(1, 1, 4, 0), (1, 2, 8, 0), (128, 125, 16, 0), (512, 625, 32, 0), (128, 625, 128, 0), (3, 7, 4, 5 * 3 + 2),
          (1, 128, 128, 0), (1, 9, 4, 3), (2, 37, 8, 2 * 2 + 1)]
_rng = np.random.default_rng(1712)
# {phase0, step}: a step of 0, phases that wrap 2^32 every few samples, steps of either sign, production-like steps
ROT16 = [(0, 0), (0xFFFFFFF0, 0x0FFFFFFF), (12345, 0xF5C28F5C), (0x80000000, 0x80000001), (7, 0xFFFFFFFF)] + \
        [tuple(int(v) for v in _rng.integers(0, 1 << 32, 2)) for _ in range(11)]
# (channels, rotation, nco_bits, out_stride - nout)
CONFIGS = [(1, False, 0, 0), (1, True, 12, 3), (3, True, 1, 0), (16, True, 20, 9)]
_cache = {}


def stream(n, seed=0):
    key = ("x", n, seed)
    if key not in _cache:
        rng = np.random.default_rng(900 + seed)
        _cache[key] = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5)
    return _cache[key]


def taps_of(L, T):
    if ("g", L, T) not in _cache:
        _cache[("g", L, T)] = random_taps(np.random.default_rng(L * 131 + T), L, T)
    return _cache[("g", L, T)]


def in_format(x, fmt):
    """-> (what the device gets: complex64 (n,) or raw (n, 2), the floats of the definition, scale)"""
    if fmt == IQ_F32:
        f = np.asarray(x, np.complex64)
        return f, f, 1.0
    raw, scale = quantise(x, fmt)
    return raw, convert_model(raw, fmt, scale), scale


def needed(r, nout, n):
    """bool (n,): the samples some output of the call reads"""
    need = np.zeros(n + 1, np.int64)
    P = r.pos0 + np.arange(nout, dtype=np.int64) * r.M
    np.add.at(need, P // r.L, 1)
    np.add.at(need, P // r.L + r.T, -1)
    return np.cumsum(need)[:n] > 0


def poisoned(dev_samples, fmt, keep):
    out = dev_samples.copy()
    if fmt == IQ_F32:
        out[~keep] = complex(np.nan, np.nan)
    else:
        out[~keep] = ~out[~keep]
    return out


def upload(dev_samples, fmt):
    """at the least alignment the format may have: 8 bytes for float32, 4 for the integer formats"""
    if fmt != IQ_F32:
        return dev_raw(dev_samples)
    t = torch.empty(dev_samples.size + 1, dtype=torch.complex64, device="cuda")
    d = t[1:]
    d.copy_(torch.from_numpy(np.ascontiguousarray(dev_samples)))
    assert d.data_ptr() % 16 == 8
    return d


def dev_tables(V, r):
    d_taps = torch.from_numpy(r.taps).cuda()
    d_nco = None if r.rot is None else nco_tables(V, r.nco_bits)[1]
    return d_taps, d_nco


def run(V, dev_samples, floats, fmt, scale, r, nout, slack=0, extra_stride=0, stream_=None, check=True):
    """one call on a sentinel-filled output; -> the model's (nchan, nout).  nsamples = the last needed sample + 1 + slack;
    every sample no output needs is poisoned on the device"""
    want = resample_model(floats, r, nout)
    last = (r.pos0 + (nout - 1) * r.M) // r.L + r.T if nout else 0
    ns = min(last + slack, floats.size)
    keep = needed(r, nout, dev_samples.shape[0])
    d_iq = upload(poisoned(dev_samples, fmt, keep), fmt)
    if fmt == IQ_CU8 and nout and (r.pos0 // r.L) % 2:
        assert (d_iq.data_ptr() + 2 * (r.pos0 // r.L)) % 4 == 2
    d_taps, d_nco = dev_tables(V, r)
    stride = nout + extra_stride
    image = np.full(2 * GW + (r.nchan - 1) * stride + nout, SENT + 0j, np.complex64)
    d_out = torch.from_numpy(image).cuda()
    V.iq_resample_dev(d_iq, r.L, r.M, d_taps, nout, d_out[GW:], pos0=r.pos0, rot=r.rot, d_nco=d_nco, nco_bits=r.nco_bits,
                      out_stride=stride, nsamples=ns, stream=stream_, iq_format=fmt, iq_scale=scale)
    for c in range(r.nchan):
        image[GW + c * stride:GW + c * stride + nout] = want[c]
    if not check:
        return want, d_out, image
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    bad = np.flatnonzero((got.real != image.real) | (got.imag != image.imag))
    assert bad.size == 0, "outputs, gaps and guards: first differences at %s of %d" % (bad[:8].tolist(), image.size)
    return want


def rs_of(shape, cfg):
    L, M, T, pos0 = shape
    nchan, rot, bits, _ = cfg
    return Rs(L, M, taps_of(L, T), pos0, ROT16[:nchan] if rot and nchan > 1 else ([ROT16[2]] if rot else None), bits)


@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_against_the_model(V, torch_cuda, shape):
    """nout 1, one less than, equal to and one more than the tile, three tiles and a remainder, and exactly what the stream
    holds - each with another format and channel configuration; then every format with every configuration"""
    L, M, T, pos0 = shape
    tile, direct = V.resample_tile(L, M, T)
    assert direct == (M > L * T)
    n = (pos0 + (3 * tile + 41) * M) // L + T + 16
    x = stream(n)
    ins = [in_format(x, fmt) for fmt in FORMATS]
    full = out_count_model(n - 9, L, M, T, pos0)
    assert full > 3 * tile + 7
    for i, nout in enumerate((1, tile - 1, tile, tile + 1, 3 * tile + 7, full)):
        if nout == 0:
            continue
        for j in (i, i + 1):
            fmt, cfg = FORMATS[j % 4], CONFIGS[(i + j // 4) % 4]
            dev, floats, scale = ins[fmt]
            run(V, dev, floats, fmt, scale, rs_of(shape, cfg), nout, slack=0 if nout == full else 5, extra_stride=cfg[3])
    for fmt in FORMATS:
        dev, floats, scale = ins[fmt]
        for cfg in CONFIGS:
            run(V, dev, floats, fmt, scale, rs_of(shape, cfg), tile + 1 if tile > 1 else 3, slack=2, extra_stride=cfg[3])


def test_p_beyond_32_bits(V, torch_cuda):
    """(1024, 4096, 4) with a little over 2^20 outputs of about 4 M CU8 samples: P = m*M passes 2^32, and the grid has more
    tiles than a workgroup's first"""
    L, M, T = 1024, 4096, 4
    nout = (1 << 20) + 37
    n = ((nout - 1) * M) // L + T
    assert (nout - 1) * M > 1 << 32
    dev, floats, scale = in_format(stream(n, seed=1), IQ_CU8)
    r = Rs(L, M, taps_of(L, T), 0, [ROT16[2], ROT16[1]], 12)
    want = run(V, dev, floats, IQ_CU8, scale, r, nout, extra_stride=1)
    assert np.abs(want).max() > 0.1


def test_continuation_on_the_device(V, torch_cuda):
    """two calls by the header's rule - the second on the buffer without its first s samples - equal one long call"""
    for shape, cfg, fmt in ((SHAPES[3], CONFIGS[2], IQ_F32), (SHAPES[5], CONFIGS[1], IQ_CU8), (SHAPES[4], CONFIGS[3], IQ_CS16)):
        L, M, T, pos0 = shape
        tile = V.resample_tile(L, M, T)[0]
        nout, m1 = tile + 300, tile // 2 + 3
        n = (pos0 + nout * M) // L + T + 1
        dev, floats, scale = in_format(stream(n, seed=2), fmt)
        r = rs_of(shape, cfg)
        whole = run(V, dev, floats, fmt, scale, r, nout)
        s, r2 = continuation(r, m1)
        assert s > 0
        first = run(V, dev, floats, fmt, scale, r, m1)
        second = run(V, dev[s:], floats[s:], fmt, scale, r2, nout - m1)
        assert np.array_equal(np.concatenate([first, second], axis=1).view(np.uint32), whole.view(np.uint32))


def test_all_zero_stream_and_nothing_to_do(V, torch_cuda):
    """an all-zero CS16 stream gives zeros in every channel (rotation on); nout = 0 writes nothing"""
    z = np.zeros((3000, 2), np.int16)
    r = rs_of(SHAPES[3], CONFIGS[2])
    want = run(V, z, convert_model(z, IQ_CS16, 2.0 ** -15), IQ_CS16, 2.0 ** -15, r, 1500, extra_stride=4)
    assert not want.any()
    d_out = torch.full((64,), complex(float(SENT), float(SENT)), dtype=torch.complex64, device="cuda")
    d_taps, d_nco = dev_tables(V, r)
    V.iq_resample_dev(dev_raw(z), r.L, r.M, d_taps, 0, d_out, rot=r.rot, d_nco=d_nco, nco_bits=r.nco_bits, iq_format=IQ_CS16,
                      iq_scale=2.0 ** -15)
    torch.cuda.synchronize()
    assert bool((d_out == complex(float(SENT), float(SENT))).all())


def test_argument_errors(V, torch_cuda):
    assert replay_argument_errors(V, torch) >= 35


def test_two_streams(V, torch_cuda):
    """two calls back to back on two streams with different parameters: each equals its result alone"""
    a = (SHAPES[3], CONFIGS[3], IQ_CU8)
    b = (SHAPES[2], CONFIGS[1], IQ_F32)
    jobs = []
    for k, (shape, cfg, fmt) in enumerate((a, b)):
        L, M, T, pos0 = shape
        nout = 5 * V.resample_tile(L, M, T)[0] + 11
        dev, floats, scale = in_format(stream((pos0 + nout * M) // L + T + 1, seed=3 + k), fmt)
        jobs.append((dev, floats, fmt, scale, rs_of(shape, cfg), nout, cfg[3]))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    pending = []
    for (dev, floats, fmt, scale, r, nout, extra), s in zip(jobs, streams):
        with torch.cuda.stream(s):  # the uploads and the call on one stream
            pending.append(run(V, dev, floats, fmt, scale, r, nout, extra_stride=extra, stream_=s.cuda_stream, check=False))
    torch.cuda.synchronize()
    for want, d_out, image in pending:
        got = d_out.cpu().numpy()
        assert np.array_equal(got.real, image.real) and np.array_equal(got.imag, image.imag)


def test_end_to_end_into_the_demodulator(V, O, torch_cuda):
    """a 2.5 MS/s CU8 stream of three frame periods, 200 kHz off: vit_iq_resample_dev -> vit_ofdm_acquire_dev ->
    vit_ofdm_sync_dev -> vit_ofdm_demod_dev with nothing leaving the device.  The FIC bytes are identical to those of the
    same calls on the model's resampled floats."""
    x, _, prs, bins = chain_case(O)
    r, a, prm = chain_params(V)
    raw, scale = quantise(x, IQ_CU8)
    floats = convert_model(raw, IQ_CU8, scale)
    nout = out_count_model(floats.size, r.L, r.M, r.T)
    want = resample_model(floats, r, nout)[0]
    d_taps, d_nco = dev_tables(V, r)
    d_y = torch.full((nout,), complex(float(SENT), float(SENT)), dtype=torch.complex64, device="cuda")
    V.iq_resample_dev(dev_raw(raw), r.L, r.M, d_taps, nout, d_y, rot=r.rot, d_nco=d_nco, nco_bits=r.nco_bits, iq_format=IQ_CU8,
                      iq_scale=scale)
    nfft, nsyms, n, K = prm.nfft, prm.nsyms, CHAIN_FRAMES, MODE_I[1]
    d_tw, d_prs, d_bins = tw_tables(V, nfft)[1], torch.from_numpy(prs).cuda(), dev_bins(bins)

    def chain(d_iq):
        d_start = torch.full((n,), -7, dtype=torch.int64, device="cuda")
        V.ofdm_acquire_dev(d_iq, a.B, a.Ln, a.Lr, a.Pb, a.thr, n, d_start, offset=a.offset)
        d_rot = dev_u32(np.zeros((n, 2), np.uint32))
        V.ofdm_sync_dev(d_iq, nfft, nsyms, n, d_tw, prm.sym_stride, d_nco, 12, d_prs, d_start, d_rot, prm.W, prm.M,
                        cp_symbols=prm.cp_symbols, thr=prm.thr, backoff=prm.backoff, d_start=d_start)
        d_fic = torch.full((n, 3 * 2 * K), 77, dtype=torch.uint8, device="cuda")
        V.ofdm_demod_dev(d_iq, MODE_I, d_bins, 254.0, n, d_tw, prm.sym_stride, d_start=d_start, d_nco=d_nco, nco_bits=12,
                         d_rot=d_rot, d_fic=d_fic)
        torch.cuda.synchronize()
        return d_start.cpu().numpy(), d_rot.cpu().numpy(), d_fic.cpu().numpy()

    got = chain(d_y)
    assert np.array_equal(d_y.cpu().numpy(), want)
    ref = chain(torch.from_numpy(want).cuda())
    assert (got[0] >= 0).all() and np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    assert np.array_equal(got[0], acquire_and_sync_starts(want, a, prm, prs))
    assert np.array_equal(got[2], ref[2]), "FIC bytes"
    assert (got[2] != 77).mean() > 0.9


def acquire_and_sync_starts(y, a, prm, prs):
    """the models' fine starts on the resampled floats"""
    from test_fft_host import nco_model, twiddles_model
    from test_sync_host import sync_model
    coarse = acquire_model(y, a, CHAIN_FRAMES)[0]
    return sync_model(y, coarse, prm, prs, twiddles_model(prm.nfft), nco_model(12), 12)[0]
