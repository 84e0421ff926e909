"""GPU: "From the stream: first acquisition" - vit_ofdm_acquire_dev against the numpy float32 model of
tests/test_acq_host.py in every output word (the starts, the 4 info words, the block powers when asked for), in guarded
buffers compared whole: the block lengths and windows at which the kernels take another path, period counts 1, 3 and 70,
`first` 0 and odd (a CU8 block at an address that is 2 mod 4), the four sample formats, d_info and d_power each absent and
given, the tie, the all-zero stream, the empty and the partial period, a stream that ends in mid-block in front of
samples that must not be read, the argument rules, and end to end through vit_ofdm_sync_dev into vit_ofdm_demod_dev."""
import numpy as np
import pytest
import torch  # noqa: F401  (torch's runtime first, as when the whole suite is collected)

from test_acq_host import NOISE_PERIODS, NONE, Acq, acquire_model, argument_error_cases, noise_case
from test_gpu_iqfmt import dev_raw
from test_gpu_ofdm import dev_bins
from test_gpu_ofdm_td import dev_u32, nco_tables, tw_tables
from test_iqfmt_host import INT_FORMATS, IQ_CS8, IQ_CS16, IQ_CU8, convert_model, quantise
from test_sync_host import std_bins

pytestmark = pytest.mark.gpu

IQ_F32 = 0
FORMATS = (IQ_F32,) + INT_FORMATS
SENT64, SENT32 = -0x0123456789ABCDEF, 0x5A5A5A5A
GW = 3  # guard entries around every output table
# (B, Ln, Lr, Pb, nperiods): a tree inside a lane; the production block length; a tree wider than a wavefront's lanes
# hold; windows longer than a wavefront; a period that cannot sit in LDS at once
SHAPES = [(8, 2, 1, 48, 3), (32, 5, 3, 40, 4), (512, 3, 2, 7, 3), (8, 300, 170, 1000, 3), (8, 4, 4, 50000, 2)]
_cache = {}


def make_stream(shape, zero_nulls=False):
    """Gaussian samples of unit power with one null per period - exact zeros, or 40 dB down - that ends anywhere in a
    block among the period's candidates; period 1 of three and more has none.  The stream holds every period whole from
    first = 0 or 1 on and ends in mid-block -> complex128 (n,), built once"""
    key = (shape, zero_nulls)
    if key not in _cache:
        B, Ln, Lr, Pb, nper = shape
        rng = np.random.default_rng(700 + B + Ln + Pb + nper)
        n = (nper * Pb + Ln + Lr) * B + B // 2 + 3
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5)
        null = (Ln + 1) * B  # wherever the edge lies in its block, the Ln blocks in front of that block are inside the null
        for k in range(nper):
            if k == 1 and nper > 2:
                continue
            edge = (Ln + k * Pb) * B + int(rng.integers(B, (Pb - Lr) * B))
            x[edge - null:edge] *= 0.0 if zero_nulls else 0.01
        _cache[key] = x
    return _cache[key]


def in_format(x, fmt):
    """-> (what the device gets: complex64 (n,) or raw (n, 2), the floats of the definition, scale)"""
    if fmt == IQ_F32:
        f = np.asarray(x, np.complex64)
        return f, f, 1.0
    raw, scale = quantise(x, fmt)
    return raw, convert_model(raw, fmt, scale), scale


def run_acq(V, dev_samples, floats, fmt, scale, a, nperiods, with_info=True, with_power=True, nsamples=None):
    """one call on guarded outputs; the whole buffers are compared with the model's image, bit for bit -> the model's
    (start, info, p).  floats: what the model reads; samples at and beyond nsamples belong to the buffer only"""
    n = floats.size if nsamples is None else nsamples
    start, info, p = acquire_model(floats, a, nperiods, nsamples=n)
    if fmt == IQ_F32:
        d_iq = torch.from_numpy(np.ascontiguousarray(dev_samples)).cuda()
        assert d_iq.data_ptr() % 16 == 0
    else:
        d_iq = dev_raw(dev_samples)  # 4 bytes behind an allocation: the least alignment an integer format may have
        if fmt != IQ_CS16 and a.first % 2:
            assert (d_iq.data_ptr() + 2 * a.first) % 4 == 2
    so = torch.full((2 * GW + nperiods,), SENT64, dtype=torch.int64, device="cuda")
    io = dev_u32(np.full(2 * GW + 4 * nperiods, SENT32, np.uint32))
    po = dev_u32(np.full(2 * GW + p.size, SENT32, np.uint32)).view(torch.float32)
    V.ofdm_acquire_dev(d_iq, a.B, a.Ln, a.Lr, a.Pb, a.thr, nperiods, so[GW:], first=a.first, offset=a.offset,
                       d_info=io[GW:] if with_info else None, d_power=po[GW:GW + p.size] if with_power else None, nsamples=n,
                       iq_format=fmt, iq_scale=scale)
    torch.cuda.synchronize()
    want_so = np.full(so.numel(), SENT64, np.int64)
    want_so[GW:GW + nperiods] = start
    want_io = np.full(io.numel(), SENT32, np.uint32)
    if with_info:
        want_io[GW:GW + 4 * nperiods] = info.reshape(-1)
    want_po = np.full(po.numel(), SENT32, np.uint32)
    if with_power:
        want_po[GW:GW + p.size] = p.view(np.uint32)
    assert np.array_equal(po.cpu().numpy().view(np.uint32), want_po), "block powers and their guards"
    assert np.array_equal(io.cpu().numpy().view(np.uint32), want_io), "info words and their guards"
    assert np.array_equal(so.cpu().numpy(), want_so), "starts and their guards"
    return start, info, p


def behind(dev_samples, fmt, nsamples):
    """the buffer with everything at and beyond nsamples replaced: NaN, or the codes' complements"""
    out = dev_samples.copy()
    if fmt == IQ_F32:
        out[nsamples:] = complex(np.nan, np.nan)
    else:
        out[nsamples:] = ~out[nsamples:]
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_against_the_model(V, torch_cuda, shape):
    """every format from first = 0 and from an odd sample, all the shape's periods and fewer, with and without d_info and
    d_power, and the stream cut in mid-block so that the last period is partial - the samples behind the cut changed"""
    B, Ln, Lr, Pb, nper = shape
    x = make_stream(shape)
    hits = 0
    for fmt in FORMATS:
        dev, floats, scale = in_format(x, fmt)
        for first in (0, 1):
            a = Acq(B, Ln, Lr, Pb, first=first, offset=B // 2 - 7)
            start, info, _ = run_acq(V, dev, floats, fmt, scale, a, nper, with_info=first == 0, with_power=first == 1)
            assert (info[:, 0] != NONE).all()
            hits += int((start != -1).sum())
        a = Acq(B, Ln, Lr, Pb, first=3, offset=-1000)
        run_acq(V, dev, floats, fmt, scale, a, 1, with_power=False)
        cut = ((nper - 1) * Pb + Ln + Lr + Pb // 2) * B + 3 + B // 2
        start, info, p = run_acq(V, behind(dev, fmt, cut), floats, fmt, scale, a, nper + 1, nsamples=cut)
        assert info[nper - 1, 0] != NONE and info[nper, 0] == NONE and p.size == (cut - 3) // B
    assert hits >= 8 * (nper - 1)  # the nulls are found: every period but the one without


def test_seventy_periods(V, torch_cuda):
    """more periods than a CU holds workgroups, in every format; the first 3 of them alone give the same words"""
    shape = (8, 2, 1, 48, 70)
    x = make_stream(shape)
    for fmt in FORMATS:
        dev, floats, scale = in_format(x, fmt)
        a = Acq(8, 2, 1, 48, first=fmt % 2, offset=5)
        s70, i70, _ = run_acq(V, dev, floats, fmt, scale, a, 70)
        s3, i3, _ = run_acq(V, dev, floats, fmt, scale, a, 3, with_power=False)
        assert np.array_equal(s70[:3], s3) and np.array_equal(i70[:3], i3)


@pytest.mark.parametrize("fmt", (IQ_F32, IQ_CS8, IQ_CS16))
def test_ties_and_the_all_zero_stream(V, torch_cuda, fmt):
    """nulls of exact zeros: every candidate in front of the edge ties at q = 0 and the last wins, across threads,
    wavefronts and LDS tiles; two such nulls in one period: the later one; the all-zero stream: q = +Inf everywhere, the
    period's last candidate, start -1.  (No CU8 sample is 0.)"""
    for shape in (SHAPES[0], SHAPES[3], SHAPES[4]):
        B, Ln, Lr, Pb, nper = shape
        dev, floats, scale = in_format(make_stream(shape, zero_nulls=True), fmt)
        start, info, _ = run_acq(V, dev, floats, fmt, scale, Acq(B, Ln, Lr, Pb), nper)
        nulls = np.arange(nper) != (1 if nper > 2 else -1)
        assert (start[nulls] != -1).all() and not info[nulls, 1].any()
    rng = np.random.default_rng(61)
    B, Ln, Lr, Pb = 8, 2, 2, 40
    x = rng.standard_normal(Pb * B) + 1j * rng.standard_normal(Pb * B)
    x[5 * B:9 * B] = 0
    x[20 * B + 3:26 * B + 5] = 0
    dev, floats, scale = in_format(x, fmt)
    assert run_acq(V, dev, floats, fmt, scale, Acq(B, Ln, Lr, Pb), 1)[0][0] == 26 * B
    inf = int(np.array([np.inf], np.float32).view(np.uint32)[0])
    for B, Ln, Lr, Pb, n in ((8, 3, 2, 10, 25 * 8 + 5), (512, 1, 1, 3, 14 * 512), (8, 4, 4, 3000, 7000 * 8)):
        z = np.zeros(n, np.complex128)
        z[0] = 1.0  # quantise scales by the largest component; block 0 is in front of every R
        dev, floats, scale = in_format(z, fmt)
        start, info, _ = run_acq(V, dev, floats, fmt, scale, Acq(B, Ln, Lr, Pb, first=8 * B), 4)
        assert (start == -1).all() and (info[:, 1] == inf).all() and not info[:, 2:].any()
        assert info[0, 0] == min(Pb, n // B - 8 - Ln - Lr + 1) - 1


def test_nothing_to_search(V, torch_cuda):
    """nblk = 0 (first = nsamples, fewer samples than a block), too few blocks for one candidate, periods beyond the
    stream: start -1 and info {0xFFFFFFFF, +Inf, 0, 0}; the powers that exist are still written"""
    x = make_stream(SHAPES[0])
    for fmt in (IQ_F32, IQ_CU8):
        dev, floats, scale = in_format(x, fmt)
        for first, n in ((40, 40), (0, 7), (5, 5 + 2 * 8 + 7), (0, 48 * 8)):
            start, info, _ = run_acq(V, dev, floats, fmt, scale, Acq(8, 2, 1, 48, first=first), 3, nsamples=n)
            assert start[1:].tolist() == [-1, -1] and (info[1:, 0] == NONE).all()
    # far more periods than the stream holds
    dev, floats, scale = in_format(x, IQ_F32)
    start, info, _ = run_acq(V, dev, floats, IQ_F32, scale, Acq(8, 2, 1, 48), 300, with_power=False)
    assert (info[:4, 0] != NONE).all() and (info[4:, 0] == NONE).all()  # the stream's last block is one candidate more


def test_argument_errors(V, torch_cuda):
    assert argument_error_cases(V, torch) >= 30


def test_end_to_end_into_the_demodulator(V, torch_cuda):
    """the noise test's stream: vit_ofdm_acquire_dev writes the coarse table, vit_ofdm_sync_dev reads it as in->d_start and
    writes the two tables vit_ofdm_demod_dev reads - nothing leaves the device in between.  The FIC bytes and the ring
    rows equal those of the same chain started from the true starts."""
    x, true, prs, prm, a = noise_case()
    nfft, nsyms, n, nco_bits = prm.nfft, prm.nsyms, NOISE_PERIODS, 12
    shape = (nfft, 3 * nfft // 4, nsyms, 3, 2)
    K, per = shape[1], (nsyms - 1 - 3) // 2
    d_iq = torch.from_numpy(x).cuda()
    d_tw, d_nco = tw_tables(V, nfft)[1], nco_tables(V, nco_bits)[1]
    d_prs, d_bins = torch.from_numpy(prs).cuda(), dev_bins(std_bins(nfft))

    def chain(d_start):
        d_rot = dev_u32(np.zeros((n, 2), np.uint32))
        V.ofdm_sync_dev(d_iq, nfft, nsyms, n, d_tw, prm.sym_stride, d_nco, nco_bits, d_prs, d_start, d_rot, prm.W, prm.M,
                        thr=prm.thr, backoff=prm.guard // 2, d_start=d_start)
        d_fic = torch.full((n, 3 * 2 * K), 77, dtype=torch.uint8, device="cuda")
        d_ring = torch.full((n * 2, per * 2 * K), 77, dtype=torch.uint8, device="cuda")
        V.ofdm_demod_dev(d_iq, shape, d_bins, 254.0, n, d_tw, prm.sym_stride, d_start=d_start, d_nco=d_nco, nco_bits=nco_bits,
                         d_rot=d_rot, d_fic=d_fic, d_ring=d_ring)
        torch.cuda.synchronize()
        return d_start.cpu().numpy(), d_rot.cpu().numpy(), d_fic.cpu().numpy(), d_ring.cpu().numpy()

    d_table = torch.full((n,), SENT64, dtype=torch.int64, device="cuda")
    V.ofdm_acquire_dev(d_iq, a.B, a.Ln, a.Lr, a.Pb, a.thr, n, d_table, offset=a.offset)
    got = chain(d_table)
    want = chain(torch.from_numpy(true).cuda())
    assert np.array_equal(got[0], true - prm.guard // 2) and np.array_equal(want[0], got[0])
    assert np.array_equal(got[2], want[2]), "FIC bytes"
    assert np.array_equal(got[3], want[3]), "ring rows"
    assert (got[2] != 77).mean() > 0.9 and (got[3] != 77).mean() > 0.9  # written: 77 is one soft value of 256
