"""GPU: "From the samples" - vit_ofdm_fft_dev against the numpy float32 model of tests/test_fft_host.py in every float (by
value), vit_ofdm_demod_dev byte-exact against demap_model(fft_model(rotate_model(...))) in guarded, poisoned buffers
compared whole, the two calls against each other with no model in the loop, skipped frames, argument errors, a batch of
three times what the device holds, and end to end from a time-domain transmitter into vit_decode_fic_dev and
vit_dabplus_ti_superframes_dev."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (torch's runtime first, as when the whole suite is collected)

from test_dab_host import scramble
from test_fft_host import LENGTHS, cfo_step, front_model, time_domain
from test_gpu_dab import dabplus_superframes, decodable_segments
from test_gpu_ofdm import FIC_GUARD, GUARD, ODD_SHAPES, POISON, ceil_div, dev_bins, subset_bins
from test_ofdm_host import (MODE_I, MODE_II, MODE_III, MODE_IV, demap_model, fic_bits, freq_bins_model, random_carrier_gain,
                            split_model, transmit)
from test_punct_host import fic_segments, puncture
from test_ti_host import interleave

pytestmark = pytest.mark.gpu

NAN = np.complex64(complex(np.nan, np.nan))
GUARDS = {2048: 504, 512: 126, 256: 63, 1024: 252}  # the four modes' guard intervals in samples
STEPS = (0, 1, 1 << 31, (1 << 32) - 1)
_tables = {}


def tw_tables(V, nfft):
    """host and device copies of the library's twiddles, built once"""
    if ("tw", nfft) not in _tables:
        host = V.fft_twiddles(nfft)
        _tables[("tw", nfft)] = (host, torch.from_numpy(host).cuda())
    return _tables[("tw", nfft)]


def nco_tables(V, nco_bits):
    if ("nco", nco_bits) not in _tables:
        host = V.nco_table(nco_bits)
        _tables[("nco", nco_bits)] = (host, torch.from_numpy(host).cuda())
    return _tables[("nco", nco_bits)]


def dev_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda()


def place(parts, starts, sym_stride, nsamples):
    """useful parts (nframes, nsyms, nfft) at samples starts[t] + l*sym_stride of a buffer of nsamples, NaN everywhere else"""
    buf = np.full(nsamples, NAN, np.complex64)
    nfft = parts.shape[2]
    for t in range(parts.shape[0]):
        for l in range(parts.shape[1]):
            o = int(starts[t]) + l * sym_stride
            buf[o:o + nfft] = parts[t, l]
    return buf


class Layout:
    """where the frames are: uniform strides (d_start NULL) or a table of irregular, odd sample positions; the buffer
    ends with the last read sample"""

    def __init__(self, rng, nframes, nsyms, nfft, table, sym_stride=None):
        self.sym_stride = nfft + int(rng.integers(0, 40)) if sym_stride is None else sym_stride
        extent = (nsyms - 1) * self.sym_stride + nfft
        if table:
            gaps = rng.integers(0, 30, nframes) * 2 + 1
            order = rng.permutation(nframes)  # the frames need not be in order
            pos = np.zeros(nframes, np.int64)
            pos[order] = np.cumsum(gaps) + np.arange(nframes) * extent
            self.starts, self.frame_stride = pos, 0
        else:
            self.frame_stride = extent + int(rng.integers(0, 60))
            self.starts = np.arange(nframes, dtype=np.int64) * self.frame_stride
        self.nsamples = int(self.starts.max()) + extent
        self.d_start = torch.from_numpy(self.starts).cuda() if table else None

    def args(self):
        return dict(sym_stride=self.sym_stride, frame_stride=self.frame_stride, d_start=self.d_start)


class Rotation:
    """None, or nco_bits and a per-frame table of {phase0, step}"""

    def __init__(self, V, rng, nframes, nco_bits, steps=None):
        self.nco_bits = nco_bits
        self.rot = None
        self.nco = self.d_nco = self.d_rot = None
        if nco_bits:
            self.nco, self.d_nco = nco_tables(V, nco_bits)
            steps = [STEPS[int(rng.integers(0, 4))] if rng.random() < 0.5 else int(rng.integers(0, 1 << 32))
                     for _ in range(nframes)] if steps is None else steps
            self.rot = np.array([[int(rng.integers(0, 1 << 32)), s] for s in steps], np.uint32)
            self.d_rot = dev_u32(self.rot)

    def args(self, V, nfft):
        return dict(d_tw=tw_tables(V, nfft)[1], d_nco=self.d_nco, nco_bits=self.nco_bits, d_rot=self.d_rot)

    def model(self, V, parts, sym_stride):
        tw = tw_tables(V, parts.shape[2])[0]
        return front_model(parts, tw, self.nco, self.nco_bits, self.rot, sym_stride)


def samples_family(name, rng, nframes, nsyms, nfft):
    """time-domain inputs inside the header's domain"""
    shape = (nframes, nsyms, nfft)
    if name == "gauss":
        x = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    elif name == "spread":
        # every component 0 or of magnitude 2^-40 ... 2^40
        def comp():
            v = rng.uniform(1.0, 2.0, shape) * 2.0 ** rng.integers(-40, 40, shape) * rng.choice([-1.0, 1.0], shape)
            return np.where(rng.random(shape) < 0.1, 0.0, v)
        x = comp() + 1j * comp()
    elif name == "tones":
        x = np.zeros(shape, np.complex128)
        for t in range(nframes):
            for l in range(nsyms):
                if (t + l) % 2:  # an impulse
                    x[t, l, int(rng.integers(0, nfft))] = complex(rng.standard_normal(), rng.standard_normal())
                else:            # a single tone
                    k = int(rng.integers(0, nfft))
                    x[t, l] = np.exp(2j * np.pi * k * np.arange(nfft) / nfft) * rng.uniform(0.5, 2.0)
    else:
        raise ValueError(name)
    return x.astype(np.complex64)


# ---- vit_ofdm_fft_dev -----------------------------------------------------------------------------------------------

def run_fft_case(V, rng, parts, lay, rot):
    nframes, nsyms, nfft = parts.shape
    d_iq = torch.from_numpy(place(parts, lay.starts, lay.sym_stride, lay.nsamples)).cuda()
    oss = nfft + 2 * int(rng.integers(0, 5))
    ofs = nsyms * oss + 2 * int(rng.integers(0, 9))
    out_n = (nframes - 1) * ofs + (nsyms - 1) * oss + nfft
    d_fft = torch.full((out_n + 4,), complex(float("nan"), float("nan")), dtype=torch.complex64, device="cuda")
    V.ofdm_fft_dev(d_iq, nfft, nsyms, nframes, d_fft=d_fft, out_sym_stride=oss, out_frame_stride=ofs, **lay.args(),
                   **rot.args(V, nfft))
    torch.cuda.synchronize()
    got = d_fft.cpu().numpy()
    want = rot.model(V, parts, lay.sym_stride)
    written = np.zeros(got.size, bool)
    for t in range(nframes):
        for l in range(nsyms):
            o = t * ofs + l * oss
            written[o:o + nfft] = True
            g, w = got[o:o + nfft], want[t, l]
            assert np.array_equal(g.real, w.real) and np.array_equal(g.imag, w.imag), (t, l)  # by value: -0 == +0
    assert np.isnan(got[~written].real).all() and np.isnan(got[~written].imag).all(), "the gaps keep their poison"


@pytest.mark.parametrize("nfft", LENGTHS)
def test_fft_equals_the_model(V, torch_cuda, nfft):
    """every length, 1 and 3 frames of 3 to 5 symbols, every input family, without rotation and with it at nco_bits 1, 10
    and 20 (steps 0, 1, 2^31, 2^32 - 1 and random ones), uniform strides and a table of odd positions; NaN between the
    useful parts and in the gaps of the output"""
    rng = np.random.default_rng(100 + nfft)
    special = iter([list(STEPS[:3]), [STEPS[3], STEPS[0], STEPS[2]], [STEPS[1], STEPS[3], 12345]])
    for fam in ("gauss", "spread", "tones"):
        for nframes in (1, 3):
            for nco_bits in (0, 1, 10, 20):
                for table in (False, True):
                    nsyms = int(rng.integers(3, 6))
                    steps = next(special, None) if nco_bits and nframes == 3 and not table else None
                    run_fft_case(V, rng, samples_family(fam, rng, nframes, nsyms, nfft),
                                 Layout(rng, nframes, nsyms, nfft, table), Rotation(V, rng, nframes, nco_bits, steps))


def test_fft_of_a_whole_frame(V, torch_cuda):
    """76 symbols: the phase runs over the whole frame, guards included"""
    rng = np.random.default_rng(176)
    for table in (False, True):
        run_fft_case(V, rng, samples_family("gauss", rng, 2, 76, 256), Layout(rng, 2, 76, 256, table),
                     Rotation(V, rng, 2, 20, [cfo_step(0.3, 256), (1 << 32) - 1]))


# ---- vit_ofdm_demod_dev ---------------------------------------------------------------------------------------------

def run_demod_case(V, parts, bins, shape, gain, lay, rot, use_fic=True, use_ring=True, nrows=None, first_row=0, col=0,
                   extra=0, fic_offset=3, ring_offset=1, skipped=()):
    """one call on poisoned, guarded buffers at odd offsets; the whole buffers are compared with the model's image of
    them (the frames in `skipped` keep their poison)"""
    nfft, K, nsyms, fic_syms, cifs = shape
    nframes = parts.shape[0]
    per = (nsyms - 1 - fic_syms) // cifs
    keep = [t for t in range(nframes) if t not in skipped]
    buf = place(parts[keep], lay.starts[keep], lay.sym_stride, lay.nsamples)
    d_iq = torch.from_numpy(buf).cuda()
    nrows = nframes * cifs if nrows is None else nrows
    row_bytes = col + per * 2 * K + extra
    fic_n = nframes * fic_syms * 2 * K
    fic_buf = torch.full((fic_offset + fic_n + GUARD,), FIC_GUARD, dtype=torch.uint8, device="cuda")
    ring_buf = torch.full((ring_offset + nrows * row_bytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    d_ring = ring_buf[ring_offset:ring_offset + nrows * row_bytes].view(nrows, row_bytes)
    V.ofdm_demod_dev(d_iq, shape, dev_bins(bins), gain, nframes, d_fic=fic_buf[fic_offset:] if use_fic else None,
                     d_ring=d_ring if use_ring else None, first_row=first_row, col=col, nsamples=lay.nsamples, **lay.args(),
                     **rot.args(V, nfft))
    torch.cuda.synchronize()
    want_fic = np.full(fic_buf.numel(), FIC_GUARD, np.uint8)
    want_ring = np.full(ring_buf.numel(), POISON, np.uint8)
    out = demap_model(rot.model(V, parts, lay.sym_stride), bins, shape, gain)
    mark = np.zeros_like(out)
    mark[keep] = 1  # a skipped frame's bytes stay as they were
    fic_img, ring_img = np.zeros(fic_n, np.uint8), np.zeros((nrows, row_bytes), np.uint8)
    fic_own, ring_own = np.zeros(fic_n, np.uint8), np.zeros((nrows, row_bytes), np.uint8)
    split_model(out, shape, fic=fic_img if use_fic else None, ring=ring_img if use_ring else None, first_row=first_row, col=col)
    split_model(mark, shape, fic=fic_own if use_fic else None, ring=ring_own if use_ring else None, first_row=first_row, col=col)
    want_fic[fic_offset:fic_offset + fic_n][fic_own == 1] = fic_img[fic_own == 1]
    want_ring[ring_offset:ring_offset + nrows * row_bytes].reshape(nrows, row_bytes)[ring_own == 1] = ring_img[ring_own == 1]
    assert np.array_equal(fic_buf.cpu().numpy(), want_fic), "d_fic and its guards"
    assert np.array_equal(ring_buf.cpu().numpy(), want_ring), "the ring, its poison and its guards"


def transmitted_parts(rng, bins, shape, nframes, lay_rng, cfo=0.0, snr_db=None):
    """frames of the time-domain transmitter as the receiver's useful parts, the window starting anywhere in the guard"""
    nfft, K, nsyms = shape[0], shape[1], shape[2]
    guard = GUARDS.get(nfft, nfft // 4)
    bits = rng.integers(0, 2, (nframes, nsyms - 1, 2 * K))
    z = transmit(bits, bins, shape, rng, carrier_gain=random_carrier_gain(rng, nfft), snr_db=snr_db)
    x = time_domain(z, guard, cfo)
    ss = nfft + guard
    parts = np.empty((nframes, nsyms, nfft), np.complex64)
    for t in range(nframes):
        s = int(lay_rng.integers(0, guard + 1))
        for l in range(nsyms):
            parts[t, l] = x[t, s + l * ss:s + l * ss + nfft]
    return parts, ss


@pytest.mark.parametrize("shape", [MODE_I, MODE_II, MODE_III, MODE_IV])
def test_modes_against_the_model(V, torch_cuda, shape):
    """the four transmission modes with the standard's table, 1 and 3 frames, Gaussian samples and the transmitter's, with
    and without rotation, strides and a start table, d_fic and a ring whose call rows wrap, odd col / row_bytes / offsets"""
    nfft, K, nsyms = shape[0], shape[1], shape[2]
    rng = np.random.default_rng(200 + nfft)
    bins = freq_bins_model(nfft)[1]
    for i, (nframes, fam) in enumerate(((1, "gauss"), (3, "tx"), (3, "gauss"), (1, "tx"))):
        table, nco_bits = bool(i & 1), (0, 20, 10, 1)[i]
        if fam == "tx":
            parts, ss = transmitted_parts(rng, bins, shape, nframes, rng, cfo=0.3 if nco_bits else 0.0, snr_db=10.0)
            lay = Layout(rng, nframes, nsyms, nfft, table, sym_stride=ss)
        else:
            parts = samples_family("gauss", rng, nframes, nsyms, nfft)
            lay = Layout(rng, nframes, nsyms, nfft, table)
        steps = [cfo_step(0.3, nfft)] * nframes if fam == "tx" and nco_bits else None
        nrows = nframes * shape[4] + 15 + 2
        run_demod_case(V, parts, bins, shape, 254.0, lay, Rotation(V, rng, nframes, nco_bits, steps), nrows=nrows,
                       first_row=nrows - 2, col=7, extra=4)


@pytest.mark.parametrize("shape,kind", ODD_SHAPES)
def test_odd_shapes_against_the_model(V, torch_cuda, shape, kind):
    """K = 1, odd K, tables that are not the standard's, per = 1, no FIC symbols, no CIFs, nfft 64 ... 8192; d_fic only, ring
    only, both"""
    rng = np.random.default_rng(300 + shape[0] + shape[1])
    nfft, K, nsyms, fic_syms, cifs = shape
    bins = freq_bins_model(nfft)[1] if kind == "std" else subset_bins(rng, nfft, K)
    for i, (nframes, use_fic, use_ring) in enumerate(((1, True, True), (4, True, False), (5, False, True), (2, True, True))):
        fam = ("gauss", "spread", "tones", "gauss")[i]
        gain = float(rng.choice([1.0, 127.0, 180.5, 254.0, 65536.0]))
        nrows = nframes * cifs + int(rng.integers(0, 20))
        run_demod_case(V, samples_family(fam, rng, nframes, nsyms, nfft), bins, shape, gain,
                       Layout(rng, nframes, nsyms, nfft, bool(i & 1)), Rotation(V, rng, nframes, (10, 0, 20, 1)[i]),
                       use_fic=use_fic, use_ring=use_ring, nrows=nrows, first_row=int(rng.integers(0, nrows)),
                       col=int(rng.integers(0, 40)), extra=int(rng.integers(1, 9)), fic_offset=int(rng.integers(0, 8)),
                       ring_offset=int(rng.integers(0, 8)))


def test_demod_equals_fft_then_demap(V, torch_cuda):
    """no model in the loop: vit_ofdm_demod_dev writes the bytes of vit_ofdm_fft_dev followed by vit_ofdm_demap_dev"""
    rng = np.random.default_rng(400)
    for shape in (MODE_II, (4096, 3001, 4, 1, 2)):
        nfft, K, nsyms, fic_syms, cifs = shape
        nframes = 3
        bins = freq_bins_model(nfft)[1] if nfft == 512 else subset_bins(rng, nfft, K)
        parts = samples_family("gauss", rng, nframes, nsyms, nfft)
        lay, rot = Layout(rng, nframes, nsyms, nfft, True), Rotation(V, rng, nframes, 20)
        d_iq = torch.from_numpy(place(parts, lay.starts, lay.sym_stride, lay.nsamples)).cuda()
        d_b = dev_bins(bins)
        per = (nsyms - 1 - fic_syms) // cifs
        nrows, col = nframes * cifs + 3, 5
        outs = []
        for fused in (True, False):
            d_fic = torch.full((nframes * fic_syms * 2 * K + GUARD,), FIC_GUARD, dtype=torch.uint8, device="cuda")
            d_ring = torch.full((nrows, col + per * 2 * K + 3), POISON, dtype=torch.uint8, device="cuda")
            if fused:
                V.ofdm_demod_dev(d_iq, shape, d_b, 200.0, nframes, d_fic=d_fic, d_ring=d_ring, first_row=nrows - 1, col=col,
                                 **lay.args(), **rot.args(V, nfft))
            else:
                d_fft = torch.empty((nframes, nsyms, nfft), dtype=torch.complex64, device="cuda")
                V.ofdm_fft_dev(d_iq, nfft, nsyms, nframes, d_fft=d_fft, **lay.args(), **rot.args(V, nfft))
                V.ofdm_demap_dev(d_fft, shape, d_b, 200.0, nframes, d_fic=d_fic, d_ring=d_ring, first_row=nrows - 1, col=col)
            torch.cuda.synchronize()
            outs.append((d_fic.cpu().numpy(), d_ring.cpu().numpy()))
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
        assert (outs[0][0][:-GUARD] != FIC_GUARD).any() and (outs[0][1] != POISON).any()


def test_skipped_frames(V, torch_cuda):
    """a start table with entries that are negative, that reach one sample beyond nsamples and that end exactly at it: the
    skipped frames' bytes keep their poison, the others equal the model - in both calls"""
    rng = np.random.default_rng(500)
    shape = (128, 77, 9, 2, 3)
    nfft, K, nsyms, fic_syms, cifs = shape
    bins = subset_bins(rng, nfft, K)
    nframes = 7
    lay = Layout(rng, nframes, nsyms, nfft, True)
    extent = (nsyms - 1) * lay.sym_stride + nfft
    lay.starts = np.array([-1, 5, lay.nsamples - extent + 1, lay.nsamples - extent, -(1 << 62), lay.nsamples, 1 << 62], np.int64)
    lay.d_start = torch.from_numpy(lay.starts).cuda()
    skipped = (0, 2, 4, 5, 6)
    parts = samples_family("gauss", rng, nframes, nsyms, nfft)
    rot = Rotation(V, rng, nframes, 10)
    run_demod_case(V, parts, bins, shape, 254.0, lay, rot, nrows=nframes * cifs + 2, first_row=3, col=1, extra=2, skipped=skipped)
    # the same table through vit_ofdm_fft_dev
    keep = [1, 3]
    d_iq = torch.from_numpy(place(parts[keep], lay.starts[keep], lay.sym_stride, lay.nsamples)).cuda()
    d_fft = torch.full((nframes, nsyms, nfft), complex(float("nan"), float("nan")), dtype=torch.complex64, device="cuda")
    V.ofdm_fft_dev(d_iq, nfft, nsyms, nframes, d_fft=d_fft, sym_stride=lay.sym_stride, d_start=lay.d_start, **rot.args(V, nfft))
    torch.cuda.synchronize()
    got = d_fft.cpu().numpy()
    want = rot.model(V, parts, lay.sym_stride)[keep]
    assert np.array_equal(got[keep].real, want.real) and np.array_equal(got[keep].imag, want.imag)
    rest = np.delete(got, keep, axis=0)
    assert np.isnan(rest.real).all() and np.isnan(rest.imag).all()


def test_argument_errors(V, torch_cuda):
    """every rule is VIT_ERR_ARG with a message and launches nothing; an empty batch is VIT_OK and writes nothing"""
    L = V.lib()
    shape = MODE_II
    nfft, K, nsyms = 512, 384, 76
    ss, fs = nfft + 126, 76 * (nfft + 126) + 664
    d_iq = torch.zeros(2 * (2 * fs) + 8, dtype=torch.float32, device="cuda")
    d_tw, d_nco = tw_tables(V, nfft)[1], nco_tables(V, 10)[1]
    extent = (nsyms - 1) * ss + nfft
    assert fs + extent <= 2 * fs
    d_b = dev_bins(freq_bins_model(nfft)[1])
    d_rot = dev_u32(np.zeros((2, 2), np.uint32))
    d_start = torch.zeros(2, dtype=torch.int64, device="cuda")
    d_fic = torch.full((2 * 3 * 2 * K,), 0x33, dtype=torch.uint8, device="cuda")
    d_ring = torch.full((4, 55296 + 10), 0x33, dtype=torch.uint8, device="cuda")
    d_fft = torch.full((2 * nsyms * nfft * 2,), 3.0, dtype=torch.float32, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731

    def inp(**kw):
        a = V.iq_input(d_iq, d_tw, ss, fs, nsamples=2 * fs)
        for k, v in kw.items():
            setattr(a, k, v.value if isinstance(v, C.c_void_p) else v)
        return a

    def ring(**kw):
        r = V.cif_ring(d_ring, 0)
        for k, v in kw.items():
            setattr(r, k, v)
        return C.byref(r)

    def demod(i=None, bins=P(d_b), shape=shape, gain=254.0, nframes=2, fic=P(d_fic), ring=ring(), col=0, null_in=False):
        sh = None if shape is None else C.byref(V.OfdmShape(*shape))
        return L.vit_ofdm_demod_dev(None if null_in else C.byref(i or inp()), bins, sh, gain, nframes, fic, ring, col, s)

    def fft(i=None, nfft=nfft, nsyms=nsyms, nframes=2, out=P(d_fft), oss=nfft, ofs=nsyms * nfft, null_in=False):
        return L.vit_ofdm_fft_dev(None if null_in else C.byref(i or inp()), nfft, nsyms, nframes, out, oss, ofs, s)

    rotated = dict(d_rot=P(d_rot), d_nco=P(d_nco), nco_bits=10)
    bad_inputs = [dict(d_iq=None), dict(d_tw=None), dict(d_iq=P(d_iq, 4)), dict(sym_stride=nfft - 1), dict(sym_stride=0),
                  dict(nsamples=fs + extent - 1), dict(frame_stride=2 * fs), dict(nsamples=0), dict(sym_stride=1 << 62),
                  dict(d_rot=P(d_rot)), dict(rotated, d_nco=None), dict(rotated, nco_bits=0), dict(rotated, nco_bits=21),
                  dict(frame_stride=1 << 63)]
    for kw in bad_inputs:
        for call in (demod, fft):
            assert call(inp(**kw)) == 1, kw
            assert "bad arguments" in V.last_error(), kw
    bad_demod = [dict(null_in=True), dict(bins=None), dict(shape=None), dict(fic=None, ring=None), dict(nframes=-1),
                 dict(shape=(500, 384, 76, 3, 1)), dict(shape=(32, 24, 76, 3, 1)), dict(shape=(16384, 384, 76, 3, 1)),
                 dict(shape=(512, 0, 76, 3, 1)), dict(shape=(512, 513, 76, 3, 1)), dict(shape=(512, 384, 3, 3, 1)),
                 dict(shape=(512, 384, 76, 3, 0)), dict(shape=(512, 384, 76, 3, 5)), dict(shape=(512, 384, 0, 0, 1)),
                 dict(gain=0.0), dict(gain=-1.0), dict(gain=65537.0), dict(gain=float("inf")), dict(gain=float("nan")),
                 dict(ring=ring(d_base=None)), dict(ring=ring(first_row=4)), dict(ring=ring(first_row=5)),
                 dict(nframes=5), dict(ring=ring(nrows=1)), dict(col=11), dict(ring=ring(row_bytes=55295)),
                 dict(col=(1 << 64) - 1), dict(nframes=3)]
    for kw in bad_demod:
        assert demod(**kw) == 1, kw
        assert "bad arguments" in V.last_error(), kw
    bad_fft = [dict(null_in=True), dict(out=None), dict(out=P(d_fft, 8)), dict(oss=nfft + 1), dict(ofs=nsyms * nfft + 1),
               dict(oss=nfft - 2), dict(nfft=500), dict(nfft=32), dict(nfft=16384), dict(nsyms=0), dict(nframes=-1),
               dict(nframes=3), dict(nsyms=200)]
    for kw in bad_fft:
        assert fft(**kw) == 1, kw
        assert "bad arguments" in V.last_error(), kw
    assert demod(nframes=0) == 0 and fft(nframes=0) == 0
    torch.cuda.synchronize()
    assert bool((d_fic == 0x33).all()) and bool((d_ring == 0x33).all()) and bool((d_fft == 3.0).all())
    # what is allowed: the buffer may end with the last frame's last sample; rotation; a start table ignores frame_stride
    assert demod() == 0 and demod(col=10) == 0 and demod(fic=None) == 0 and demod(ring=None) == 0 and fft() == 0
    assert demod(inp(nsamples=fs + extent)) == 0 and fft(inp(**rotated)) == 0
    assert demod(inp(d_start=P(d_start), frame_stride=1 << 63, nsamples=5)) == 0  # both frames are skipped on the device
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        V.ofdm_demod_dev(d_iq.to(torch.float64), shape, d_b, 254.0, 1, d_tw, ss, fs, d_fic=d_fic)
    with pytest.raises(ValueError):
        V.ofdm_demod_dev(d_iq, shape, d_b, 254.0, 1, d_tw, ss, d_fic=d_fic)  # neither frame_stride nor d_start
    with pytest.raises(ValueError):
        V.ofdm_fft_dev(d_iq, nfft, nsyms, 1, d_tw, ss, d_fft.to(torch.float64), frame_stride=fs)


# The launch geometry of csrc/vit_ofdm_td.hip, mirrored: a workgroup owns one frame and a run of at most 25 consecutive
# data symbols, about 8 workgroups per CU over the grid; at nfft 2048 a workgroup is 4 wavefronts and, with rotation, the
# kernel's registers are budgeted for 3 wavefronts per SIMD: a CU holds at most 3 workgroups.
def launch_geometry(nframes, nsym):
    """-> (data symbols per run, workgroups of the grid, workgroups the device can hold at once at most)"""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    rpf = min(ceil_div(8 * cus, nframes), nsym)
    run = min(ceil_div(nsym, rpf), 25)
    return run, nframes * ceil_div(nsym, run), 3 * cus


def test_large_batch(V, torch_cuda):
    """768 mode-I frames in one call (1.2 GB of samples), 32 distinct frames tiled on the device: every workgroup's run is 25
    symbols long and the grid is three times what the device holds at once; compared on the device per distinct frame"""
    shape = MODE_I
    nfft, K, nsyms, fic_syms, cifs = shape
    base_n, reps = 32, 24
    nframes = base_n * reps
    run, grid, resident = launch_geometry(nframes, nsyms - 1)
    assert run == 25 and grid >= 3 * resident, (run, grid, resident)
    rng = np.random.default_rng(600)
    bins = freq_bins_model(nfft)[1]
    ss, fs = 2552, 196608
    parts = samples_family("gauss", rng, base_n, nsyms, nfft)
    rot = Rotation(V, rng, base_n, 20)
    want = demap_model(rot.model(V, parts, ss), bins, shape, 254.0)  # (32, 75, 3072)
    frames = np.full((base_n, fs), NAN, np.complex64)
    for l in range(nsyms):
        frames[:, 2656 + 504 + l * ss:2656 + 504 + l * ss + nfft] = parts[:, l]
    d_iq = torch.from_numpy(frames).cuda().repeat(reps, 1).reshape(-1)[2656 + 504:]  # frame 0 starts at sample 0
    d_rot = dev_u32(np.tile(rot.rot, (reps, 1)))
    nrows, col, row_bytes = nframes * cifs + 15 + 6, 5, 5 + 55296 + 2
    first_row = nrows - 1000
    ring_buf = torch.full((1 + nrows * row_bytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    d_ring = ring_buf[1:1 + nrows * row_bytes].view(nrows, row_bytes)
    fic_n = nframes * 9216
    fic_buf = torch.full((3 + fic_n + GUARD,), FIC_GUARD, dtype=torch.uint8, device="cuda")
    args = rot.args(V, nfft)
    args["d_rot"] = d_rot
    V.ofdm_demod_dev(d_iq, shape, dev_bins(bins), 254.0, nframes, sym_stride=ss, frame_stride=fs, d_fic=fic_buf[3:], d_ring=d_ring,
                     first_row=first_row, col=col, **args)
    torch.cuda.synchronize()
    del d_iq
    d_want = torch.from_numpy(want).cuda()
    assert bool((fic_buf[:3] == FIC_GUARD).all()) and bool((fic_buf[3 + fic_n:] == FIC_GUARD).all())
    assert bool((fic_buf[3:3 + fic_n].view(reps, base_n, 9216) == d_want[:, :3].reshape(1, base_n, 9216)).all())
    assert bool((ring_buf[:1] == POISON).all()) and bool((ring_buf[1 + nrows * row_bytes:] == POISON).all())
    assert bool((d_ring[:, :col] == POISON).all()) and bool((d_ring[:, col + 55296:] == POISON).all())
    rows = (first_row + torch.arange(nframes * cifs, device="cuda")) % nrows
    want_rows = d_want[:, 3:].reshape(base_n * cifs, 55296)
    for r in range(reps):  # one repetition's rows at a time
        got = d_ring[rows[r * base_n * cifs:(r + 1) * base_n * cifs], col:col + 55296]
        assert bool((got == want_rows).all()), r
    other = torch.ones(nrows, dtype=torch.bool, device="cuda")
    other[rows] = False
    assert int(other.sum()) == 21 and bool((d_ring[other] == POISON).all())


# ---- end to end -----------------------------------------------------------------------------------------------------

def test_end_to_end_from_the_samples(V, O, torch_cuda):
    """no model in the loop: 10 mode-I frames from the time-domain transmitter carrying 40 FIC coding blocks (120 FIBs) and,
    in their 40 CIFs, 5 DAB+ superframes of one time-interleaved sub-channel; a frequency-selective channel, AWGN (11 dB
    carrier SNR), a frequency offset of 0.3 carrier spacings and a start in mid-guard that differs per frame ->
    vit_ofdm_demod_dev with rotation -> vit_decode_fic_dev on d_fic and vit_dabplus_ti_superframes_dev on the ring"""
    rng = np.random.default_rng(700)
    shape = MODE_I
    nfft, K, nsyms, fic_syms, cifs = shape
    nframes, nsf, rsdims, start_cu = 10, 5, 24, 3
    guard, null, fs = 504, 2656, 196608
    ss = nfft + guard
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
    z = transmit(bits, bins, shape, rng, carrier_gain=random_carrier_gain(rng, nfft))
    x = time_domain(z, guard, cfo=0.3)  # a bin of its FFT holds nfft times the carrier
    sigma = np.sqrt(nfft * 10.0 ** (-11.0 / 10.0) / 2.0)  # 11 dB per unit carrier: noise of variance nfft per bin
    x = x + sigma * (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape))
    starts = np.array([t * fs + null + guard - int(rng.integers(150, 350)) for t in range(nframes)], np.int64)
    buf = np.full(nframes * fs, NAN, np.complex64)
    for t in range(nframes):
        o = starts[t] - (t * fs + null)  # the window's offset into the frame's samples
        for l in range(nsyms):
            buf[starts[t] + l * ss:starts[t] + l * ss + nfft] = x[t, o + l * ss:o + l * ss + nfft] / nfft
    d_tw, d_nco = tw_tables(V, nfft)[1], nco_tables(V, 20)[1]
    d_rot = dev_u32([[int(rng.integers(0, 1 << 32)), cfo_step(0.3, nfft)] for _ in range(nframes)])
    nrows, first_row, col = 44, 41, 9
    d_ring = torch.full((nrows, col + 55296 + 1), POISON, dtype=torch.uint8, device="cuda")
    d_fic = torch.full((nframes * 9216,), FIC_GUARD, dtype=torch.uint8, device="cuda")
    V.ofdm_demod_dev(torch.from_numpy(buf).cuda(), shape, dev_bins(bins), 180.0, nframes, d_tw, ss,
                     d_start=torch.from_numpy(starts).cuda(), d_nco=d_nco, nco_bits=20, d_rot=d_rot, d_fic=d_fic, d_ring=d_ring,
                     first_row=first_row, col=col)
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
