"""GPU: "Channel-state weighting" - vit_ofdm_demap_soft_dev and vit_ofdm_demod_soft_dev with VIT_SOFT_PER_SYMBOL against
the numpy float32 model of tests/test_csi_host.py in every soft byte and every level word (bit for bit), in guarded,
poisoned buffers compared whole: the shapes at the corners of the level's grouping, every destination, both sample
kinds, skipped frames, the special carriers and symbols, independence of the launch split, VIT_SOFT_PER_CARRIER against
the existing calls, the argument rules, and end to end through the echo channel into vit_decode_fic_dev."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (torch's runtime first, as when the whole suite is collected)

from test_csi_host import SOFT_PER_CARRIER, SOFT_PER_SYMBOL, demap_soft_model, echo_channel
from test_dab_host import fib_ok_model
from test_fft_host import time_domain
from test_gpu_iqfmt import dev_raw, place_raw, random_codes
from test_gpu_ofdm import FIC_GUARD, GUARD, POISON, dev_bins, nan_outside, subset_bins, upload
from test_gpu_ofdm_td import Layout, Rotation, place, samples_family, tw_tables
from test_iqfmt_host import IQ_CS16, IQ_CU8, USUAL_SCALE, convert_model
from test_ofdm_host import (fic_bits, fic_decode, freq_bins_model, random_carrier_gain, special_carriers, split_model,
                            transmit)
from test_punct_host import fic_segments

pytestmark = pytest.mark.gpu

LEVEL_POISON = np.float32(-7.25)  # no level is negative
# nfft, K, nsyms, fic_syms, cifs; bins "std" or "rand".  G = ceil(K/4) groups meet A = max(64, nfft/8) accumulators:
SHAPES = [
    ((64, 5, 6, 1, 2), "rand"),        # K no multiple of 4, 2 groups, a single wavefront
    ((64, 64, 5, 2, 1), "rand"),       # K = nfft, 16 groups < A = 64
    ((256, 192, 7, 2, 2), "std"),      # 48 groups < A = 64
    ((512, 384, 6, 1, 2), "std"),      # 96 groups: a partial second round over A = 64
    ((1024, 1024, 5, 2, 2), "rand"),   # exactly 2A groups, two wavefronts
    ((2048, 1536, 6, 1, 1), "std"),    # mode I: 384 groups over A = 256
    ((4096, 3001, 4, 1, 2), "rand"),   # the 1024-thread workgroups, A = 512, K odd
    ((8192, 8192, 3, 1, 1), "rand"),   # 16 wavefronts; the demapper's LDS beyond 64 KiB
]
shape_param = pytest.mark.parametrize("shape,kind", SHAPES, ids=["%d-%d" % s[0][:2] for s in SHAPES])
# (FIC, ring) destinations, nrows beyond the call's, first_row from the end (the call's rows wrap), odd col
VARIANTS = ((True, True, 3, 1, 7), (True, False, 0, 0, 0), (False, True, 2, 2, 5))


def the_bins(rng, shape, kind):
    return freq_bins_model(shape[0])[1] if kind == "std" else subset_bins(rng, shape[0], shape[1])


class Buffers:
    """poisoned, guarded d_fic, ring and d_level at odd offsets, and what a call should leave in them"""

    def __init__(self, shape, nframes, use_fic, use_ring, more_rows, back, col, extra=3, fic_offset=3, ring_offset=1):
        nfft, K, nsyms, fic_syms, cifs = shape
        self.shape, self.nframes, self.use_fic, self.use_ring, self.col = shape, nframes, use_fic, use_ring, col
        per = (nsyms - 1 - fic_syms) // cifs
        self.nrows = nframes * cifs + more_rows
        self.first_row = (self.nrows - back) % self.nrows
        self.row_bytes = col + per * 2 * K + extra
        self.fic_n, self.fic_offset, self.ring_offset = nframes * fic_syms * 2 * K, fic_offset, ring_offset
        self.lev_n = nframes * (nsyms - 1)
        self.fic_buf = torch.full((fic_offset + self.fic_n + GUARD,), FIC_GUARD, dtype=torch.uint8, device="cuda")
        self.ring_buf = torch.full((ring_offset + self.nrows * self.row_bytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        self.lev_buf = torch.full((1 + self.lev_n + 5,), float(LEVEL_POISON), dtype=torch.float32, device="cuda")

    def args(self, level=True):
        d_ring = self.ring_buf[self.ring_offset:self.ring_offset + self.nrows * self.row_bytes].view(self.nrows, self.row_bytes)
        return dict(d_fic=self.fic_buf[self.fic_offset:] if self.use_fic else None, d_ring=d_ring if self.use_ring else None,
                    first_row=self.first_row, col=self.col, d_level=self.lev_buf[1:] if level else None)

    def want(self, out, S, skipped=(), level=True):
        """the three buffers after a call whose model results are out (nframes, nsyms-1, 2K) and S (nframes, nsyms-1)"""
        nfft, K, nsyms, fic_syms, cifs = self.shape
        keep = [t for t in range(self.nframes) if t not in skipped]
        want_fic = np.full(self.fic_buf.numel(), FIC_GUARD, np.uint8)
        want_ring = np.full(self.ring_buf.numel(), POISON, np.uint8)
        mark = np.zeros_like(out)
        mark[keep] = 1  # a skipped frame's bytes stay as they were
        fic_img, ring_img = np.zeros(self.fic_n, np.uint8), np.zeros((self.nrows, self.row_bytes), np.uint8)
        fic_own, ring_own = np.zeros(self.fic_n, np.uint8), np.zeros((self.nrows, self.row_bytes), np.uint8)
        for src, fic, ring in ((out, fic_img, ring_img), (mark, fic_own, ring_own)):
            split_model(src, self.shape, fic=fic if self.use_fic else None, ring=ring if self.use_ring else None,
                        first_row=self.first_row, col=self.col)
        want_fic[self.fic_offset:self.fic_offset + self.fic_n][fic_own == 1] = fic_img[fic_own == 1]
        ring = want_ring[self.ring_offset:self.ring_offset + self.nrows * self.row_bytes].reshape(self.nrows, self.row_bytes)
        ring[ring_own == 1] = ring_img[ring_own == 1]
        want_lev = np.full(self.lev_buf.numel(), LEVEL_POISON, np.float32)
        if level:
            lev = want_lev[1:1 + self.lev_n].reshape(self.nframes, nsyms - 1)
            lo, hi = 0 if self.use_fic else fic_syms, nsyms - 1 if self.use_ring else fic_syms
            lev[keep, lo:hi] = S[keep, lo:hi]  # only the symbols the call demaps
        return want_fic, want_ring, want_lev

    def got(self):
        torch.cuda.synchronize()
        return self.fic_buf.cpu().numpy(), self.ring_buf.cpu().numpy(), self.lev_buf.cpu().numpy()

    def check(self, out, S, skipped=(), level=True, what=""):
        got, want = self.got(), self.want(out, S, skipped, level)
        assert np.array_equal(got[0], want[0]), "d_fic and its guards " + what
        assert np.array_equal(got[1], want[1]), "the ring, its poison and its guards " + what
        assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), "d_level and its guards " + what
        return got


def spectra(rng, bins, shape, nframes, snr_db=8.0):
    """FFT outputs of a frequency-selective channel with noise, NaN in every bin the table does not name"""
    nfft, K, nsyms = shape[0], shape[1], shape[2]
    bits = rng.integers(0, 2, (nframes, nsyms - 1, 2 * K))
    return nan_outside(transmit(bits, bins, shape, rng, carrier_gain=random_carrier_gain(rng, nfft), snr_db=snr_db), bins)


def demap_soft(V, z, bins, shape, gain, buf, level=True, rule=SOFT_PER_SYMBOL):
    nfft, nsyms = shape[0], shape[2]
    ss = nfft + 2
    fs = nsyms * ss + 6
    V.ofdm_demap_soft_dev(upload(z, shape, ss, fs), shape, dev_bins(bins), rule, gain, z.shape[0], sym_stride=ss,
                          frame_stride=fs, **buf.args(level))


# ---- the shapes at the grouping's corners ---------------------------------------------------------------------------

@shape_param
def test_demap_soft_equals_the_model(V, torch_cuda, shape, kind):
    """vit_ofdm_demap_soft_dev: 2 frames, FIC and ring / FIC only / ring only, a ring whose call rows wrap, odd col and
    offsets, gains over the rule's range; with and without d_level"""
    rng = np.random.default_rng(2000 + shape[0] + shape[1])
    bins = the_bins(rng, shape, kind)
    for i, variant in enumerate(VARIANTS):
        gain = (64.0, 128.0, 2.0 ** -24)[i] if shape[0] != 512 else (65536.0, 100.5, 1.0)[i]
        z = spectra(rng, bins, shape, 2)
        out, S = demap_soft_model(z, bins, shape, gain)
        level = i != 1 or shape[0] >= 1024
        buf = Buffers(shape, 2, *variant)
        demap_soft(V, z, bins, shape, gain, buf, level=level)
        buf.check(out, S, level=level, what=str(variant))
        assert i or (out != 128).mean() > 0.9


@shape_param
def test_demod_soft_equals_the_model(V, torch_cuda, shape, kind):
    """vit_ofdm_demod_soft_dev on float32 samples: the same geometry, without rotation and with it, frames by stride and
    by a table of odd positions"""
    nfft, K, nsyms = shape[0], shape[1], shape[2]
    rng = np.random.default_rng(2100 + nfft + K)
    bins = the_bins(rng, shape, kind)
    for i, variant in enumerate(VARIANTS):
        gain = (64.0, 128.0, 7.5)[i]
        parts = samples_family("gauss", rng, 2, nsyms, nfft)
        lay, rot = Layout(rng, 2, nsyms, nfft, bool(i & 1)), Rotation(V, rng, 2, (0, 20, 10)[i])
        out, S = demap_soft_model(rot.model(V, parts, lay.sym_stride), bins, shape, gain)
        buf = Buffers(shape, 2, *variant)
        d_iq = torch.from_numpy(place(parts, lay.starts, lay.sym_stride, lay.nsamples)).cuda()
        V.ofdm_demod_soft_dev(d_iq, shape, dev_bins(bins), SOFT_PER_SYMBOL, gain, 2, nsamples=lay.nsamples, **lay.args(),
                              **rot.args(V, nfft), **buf.args())
        buf.check(out, S, what=str(variant))


@pytest.mark.parametrize("fmt", [IQ_CU8, IQ_CS16], ids=["cu8", "cs16"])
def test_demod_soft_reads_integer_samples(V, torch_cuda, fmt):
    """cu8 and cs16 through fmt: the model on the converted floats"""
    rng = np.random.default_rng(2200 + fmt)
    for (shape, kind), nco_bits in ((SHAPES[0], 10), (SHAPES[3], 0), (SHAPES[5], 20)):
        nfft, K, nsyms = shape[0], shape[1], shape[2]
        bins = the_bins(rng, shape, kind)
        scale = USUAL_SCALE[fmt]
        parts = random_codes(rng, fmt, (2, nsyms, nfft))
        lay, rot = Layout(rng, 2, nsyms, nfft, True), Rotation(V, rng, 2, nco_bits)
        raw, _ = place_raw(parts, lay.starts, lay.sym_stride, random_codes(rng, fmt, (lay.nsamples,)))
        out, S = demap_soft_model(rot.model(V, convert_model(parts, fmt, scale), lay.sym_stride), bins, shape, 96.0)
        buf = Buffers(shape, 2, *VARIANTS[0])
        V.ofdm_demod_soft_dev(dev_raw(raw), shape, dev_bins(bins), SOFT_PER_SYMBOL, 96.0, 2, nsamples=lay.nsamples, iq_format=fmt,
                              iq_scale=scale, **lay.args(), **rot.args(V, nfft), **buf.args())
        buf.check(out, S, what=str(shape))


def test_skipped_frame_keeps_bytes_and_levels(V, torch_cuda):
    """a start table whose middle frame would read beyond nsamples: its bytes and level words keep their old values"""
    rng = np.random.default_rng(2300)
    shape, kind = SHAPES[2]
    nfft, K, nsyms = shape[0], shape[1], shape[2]
    bins = the_bins(rng, shape, kind)
    lay, rot = Layout(rng, 3, nsyms, nfft, True), Rotation(V, rng, 3, 20)
    extent = (nsyms - 1) * lay.sym_stride + nfft
    lay.starts[1] = lay.nsamples - extent + 1
    lay.d_start = torch.from_numpy(lay.starts).cuda()
    parts = samples_family("gauss", rng, 3, nsyms, nfft)
    out, S = demap_soft_model(rot.model(V, parts, lay.sym_stride), bins, shape, 64.0)
    buf = Buffers(shape, 3, *VARIANTS[0])
    d_iq = torch.from_numpy(place(parts[[0, 2]], lay.starts[[0, 2]], lay.sym_stride, lay.nsamples)).cuda()
    V.ofdm_demod_soft_dev(d_iq, shape, dev_bins(bins), SOFT_PER_SYMBOL, 64.0, 3, nsamples=lay.nsamples, **lay.args(),
                          **rot.args(V, nfft), **buf.args())
    buf.check(out, S, skipped=(1,))


@pytest.mark.parametrize("which", [1, 3, 5, 7])
def test_demap_soft_on_the_spectra_equals_demod_soft(V, torch_cuda, which):
    """no model in the loop: vit_ofdm_fft_dev then vit_ofdm_demap_soft_dev writes every byte and level word that
    vit_ofdm_demod_soft_dev writes"""
    shape, kind = SHAPES[which]
    nfft, K, nsyms = shape[0], shape[1], shape[2]
    rng = np.random.default_rng(2400 + which)
    bins, nframes = the_bins(rng, shape, kind), 3
    parts = samples_family("gauss", rng, nframes, nsyms, nfft)
    lay, rot = Layout(rng, nframes, nsyms, nfft, True), Rotation(V, rng, nframes, 20)
    d_iq = torch.from_numpy(place(parts, lay.starts, lay.sym_stride, lay.nsamples)).cuda()
    d_b = dev_bins(bins)
    bufs = [Buffers(shape, nframes, *VARIANTS[0]) for _ in range(2)]
    V.ofdm_demod_soft_dev(d_iq, shape, d_b, SOFT_PER_SYMBOL, 80.0, nframes, **lay.args(), **rot.args(V, nfft), **bufs[0].args())
    d_fft = torch.empty((nframes, nsyms, nfft), dtype=torch.complex64, device="cuda")
    V.ofdm_fft_dev(d_iq, nfft, nsyms, nframes, d_fft=d_fft, **lay.args(), **rot.args(V, nfft))
    V.ofdm_demap_soft_dev(d_fft, shape, d_b, SOFT_PER_SYMBOL, 80.0, nframes, **bufs[1].args())
    a, b = bufs[0].got(), bufs[1].got()
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert (a[0][3:-GUARD] != FIC_GUARD).any() and (a[2][1:1 + bufs[0].lev_n] > 0).all()


# ---- special carriers and symbols -----------------------------------------------------------------------------------

def test_special_carriers_and_symbols(V, torch_cuda):
    """on the device what tests/test_csi_host.py pins for the model: erased carriers (zero, 2^-70, NaN, Inf, overflow) in a
    live symbol, an all-zero symbol (level 0), a symbol whose level exceeds 2^96 and one whose level overflows to +Inf -
    through the demapper; the all-zero symbol through the fused call too"""
    rng = np.random.default_rng(2500)
    shape, kind = (256, 192, 14, 3, 2), "std"
    nfft, K, nsyms = shape[0], shape[1], shape[2]
    bins = the_bins(rng, shape, kind)
    bits = rng.integers(0, 2, (2, nsyms - 1, 2 * K))
    z = transmit(bits, bins, shape, rng, carrier_gain=random_carrier_gain(rng, nfft), snr_db=15.0)
    special_carriers(z, bins, 2)
    z[:, 5] = 0
    z[:, 8:10] *= np.float32(2.0 ** 45)
    z[1, 11:13] *= np.float32(2.0 ** 63)
    z = nan_outside(z, bins)
    out, S = demap_soft_model(z, bins, shape, 64.0)
    assert (out[:, 1:3, :6] == 128).all() and (out[:, 1:3, 6:K] != 128).any()
    assert (S[:, 4:6] == 0).all() and (S[:, 8] > 2.0 ** 96).all() and np.isfinite(S[:, 8]).all() and np.isposinf(S[1, 11])
    assert (out[:, 4:6] == 128).all() and (out[:, 8] == 128).all() and (out[1, 11] == 128).all() and (out[0, 11] != 128).any()
    buf = Buffers(shape, 2, *VARIANTS[0])
    demap_soft(V, z, bins, shape, 64.0, buf)
    buf.check(out, S)
    parts = samples_family("gauss", rng, 2, nsyms, nfft)
    parts[:, 5] = 0
    parts[1, 9] = 0
    lay, rot = Layout(rng, 2, nsyms, nfft, False), Rotation(V, rng, 2, 20)
    out, S = demap_soft_model(rot.model(V, parts, lay.sym_stride), bins, shape, 64.0)
    assert (S[:, 4:6] == 0).all() and (out[:, 4:6] == 128).all() and (S[1, 8:10] == 0).all() and (S[0, 8:10] > 0).all()
    buf = Buffers(shape, 2, *VARIANTS[0])
    d_iq = torch.from_numpy(place(parts, lay.starts, lay.sym_stride, lay.nsamples)).cuda()
    V.ofdm_demod_soft_dev(d_iq, shape, dev_bins(bins), SOFT_PER_SYMBOL, 64.0, 2, nsamples=lay.nsamples, **lay.args(),
                          **rot.args(V, nfft), **buf.args())
    buf.check(out, S)


# ---- the launch split ---------------------------------------------------------------------------------------------------

def test_bytes_and_levels_do_not_depend_on_the_launch_split(V, torch_cuda):
    """one frame of nfft 64 with 9 symbols alone (a workgroup per symbol) and as frame 300 of 512 (runs of several
    symbols): the same bytes and levels, through both calls"""
    rng = np.random.default_rng(2600)
    shape = (64, 49, 9, 2, 3)
    nfft, K, nsyms, fic_syms, cifs = shape
    bins = subset_bins(rng, nfft, K)
    nframes, at = 512, 300
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    assert -(-8 * cus // nframes) < nsyms - 1, "the batch must make runs longer than one symbol"
    parts = samples_family("gauss", rng, nframes, nsyms, nfft)
    tw = tw_tables(V, nfft)
    ss, fs = nfft + 3, nsyms * (nfft + 3) + 5
    d_b = dev_bins(bins)

    def both(p):
        n = p.shape[0]
        starts = np.arange(n, dtype=np.int64) * fs
        d_iq = torch.from_numpy(place(p, starts, ss, int(starts[-1]) + (nsyms - 1) * ss + nfft)).cuda()
        res = []
        for fused in (True, False):
            d_fic = torch.full((n, fic_syms * 2 * K), FIC_GUARD, dtype=torch.uint8, device="cuda")
            d_ring = torch.full((n * cifs, 2 * 2 * K), POISON, dtype=torch.uint8, device="cuda")
            d_lev = torch.full((n, nsyms - 1), float(LEVEL_POISON), dtype=torch.float32, device="cuda")
            if fused:
                V.ofdm_demod_soft_dev(d_iq, shape, d_b, SOFT_PER_SYMBOL, 64.0, n, tw[1], ss, fs, d_fic=d_fic, d_ring=d_ring,
                                      d_level=d_lev)
            else:
                d_fft = torch.empty((n, nsyms, nfft), dtype=torch.complex64, device="cuda")
                V.ofdm_fft_dev(d_iq, nfft, nsyms, n, tw[1], ss, d_fft, frame_stride=fs)
                V.ofdm_demap_soft_dev(d_fft, shape, d_b, SOFT_PER_SYMBOL, 64.0, n, d_fic=d_fic, d_ring=d_ring, d_level=d_lev)
            torch.cuda.synchronize()
            res.append((d_fic.cpu().numpy(), d_ring.cpu().numpy().reshape(n, -1), d_lev.cpu().numpy()))
        return res

    alone, among = both(parts[at:at + 1]), both(parts)
    out, S = demap_soft_model(Rotation(V, rng, 1, 0).model(V, parts[at:at + 1], ss), bins, shape, 64.0)
    for a, b in zip(alone, among):
        assert np.array_equal(a[0][0], b[0][at]) and np.array_equal(a[1][0], b[1][at])
        assert np.array_equal(a[2][0].view(np.uint32), b[2][at].view(np.uint32))
        assert np.array_equal(a[2][0].view(np.uint32), S[0].view(np.uint32))
        assert np.array_equal(a[0][0], out[0, :fic_syms].reshape(-1)) and np.array_equal(a[1][0], out[0, fic_syms:].reshape(-1))


# ---- VIT_SOFT_PER_CARRIER -----------------------------------------------------------------------------------------------

def test_per_carrier_rule_is_the_existing_calls(V, torch_cuda):
    """rule 0 through both new calls: byte for byte what vit_ofdm_demap_dev, vit_ofdm_demod_dev and vit_ofdm_demod_iq_dev
    write"""
    rng = np.random.default_rng(2700)
    for (shape, kind), gain in ((SHAPES[3], 254.0), (SHAPES[6], 127.0)):
        nfft, K, nsyms = shape[0], shape[1], shape[2]
        bins = the_bins(rng, shape, kind)
        d_b = dev_bins(bins)
        z = spectra(rng, bins, shape, 2)
        ss, fs = nfft + 2, nsyms * (nfft + 2) + 6
        d_fft = upload(z, shape, ss, fs)
        parts = samples_family("gauss", rng, 2, nsyms, nfft)
        lay, rot = Layout(rng, 2, nsyms, nfft, True), Rotation(V, rng, 2, 20)
        d_iq = torch.from_numpy(place(parts, lay.starts, lay.sym_stride, lay.nsamples)).cuda()
        codes = random_codes(rng, IQ_CU8, (2, nsyms, nfft))
        raw, _ = place_raw(codes, lay.starts, lay.sym_stride, random_codes(rng, IQ_CU8, (lay.nsamples,)))
        d_raw = dev_raw(raw)
        pairs = []
        for new in (True, False):
            bufs = [Buffers(shape, 2, *VARIANTS[0]) for _ in range(3)]
            a = [b.args(level=False) for b in bufs]
            if new:
                V.ofdm_demap_soft_dev(d_fft, shape, d_b, SOFT_PER_CARRIER, gain, 2, sym_stride=ss, frame_stride=fs, **a[0])
                V.ofdm_demod_soft_dev(d_iq, shape, d_b, SOFT_PER_CARRIER, gain, 2, **lay.args(), **rot.args(V, nfft), **a[1])
                V.ofdm_demod_soft_dev(d_raw, shape, d_b, SOFT_PER_CARRIER, gain, 2, iq_format=IQ_CU8, iq_scale=2.0 ** -8,
                                      **lay.args(), **rot.args(V, nfft), **a[2])
            else:
                for x in a:
                    del x["d_level"]
                V.ofdm_demap_dev(d_fft, shape, d_b, gain, 2, sym_stride=ss, frame_stride=fs, **a[0])
                V.ofdm_demod_dev(d_iq, shape, d_b, gain, 2, **lay.args(), **rot.args(V, nfft), **a[1])
                V.ofdm_demod_dev(d_raw, shape, d_b, gain, 2, iq_format=IQ_CU8, iq_scale=2.0 ** -8, **lay.args(),
                                 **rot.args(V, nfft), **a[2])
            pairs.append([b.got() for b in bufs])
        for x, y in zip(*pairs):
            assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
            assert (x[0][3:-GUARD] != FIC_GUARD).any() and (x[2] == LEVEL_POISON).all()


def test_argument_errors(V, torch_cuda):
    """the rules of vit_soft_rule and d_level are VIT_ERR_ARG with a message and launch nothing; the others' rules hold"""
    L = V.lib()
    shape = (256, 192, 7, 2, 2)
    nfft, K, nsyms = shape[0], shape[1], shape[2]
    d_fft = torch.zeros((2, nsyms, nfft), dtype=torch.complex64, device="cuda")
    d_iq = torch.zeros(2 * nsyms * nfft, dtype=torch.complex64, device="cuda")
    d_b = dev_bins(freq_bins_model(nfft)[1])
    d_tw = tw_tables(V, nfft)[1]
    buf = Buffers(shape, 2, True, True, 0, 0, 0)
    a = buf.args()
    sh = C.byref(V.OfdmShape(*shape))
    ring = C.byref(V.cif_ring(a["d_ring"], 0))
    inp = C.byref(V.iq_input(d_iq, d_tw, nfft, nsyms * nfft))
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731

    def calls(soft, level=P(a["d_level"]), bins=P(d_b)):
        sr = None if soft is None else C.byref(V.SoftRule(*soft))
        return (L.vit_ofdm_demap_soft_dev(P(d_fft), nfft, nsyms * nfft, bins, sh, sr, 2, P(a["d_fic"]), ring, 0, level, s),
                L.vit_ofdm_demod_soft_dev(inp, None, bins, sh, sr, 2, P(a["d_fic"]), ring, 0, level, s))

    bad = [dict(soft=None), dict(soft=(2, 64.0)), dict(soft=(0xFFFFFFFF, 64.0)), dict(soft=(1, 0.0)), dict(soft=(1, -64.0)),
           dict(soft=(1, 2.0 ** -25)), dict(soft=(1, 65537.0)), dict(soft=(1, float("inf"))), dict(soft=(1, float("nan"))),
           dict(soft=(0, 254.0)), dict(soft=(0, 0.0), level=None), dict(soft=(0, 65537.0), level=None),
           dict(soft=(1, 64.0), level=P(a["d_level"], 2)), dict(soft=(1, 64.0), bins=None)]
    for kw in bad:
        for rc in calls(**kw):
            assert rc == 1, kw
            assert "bad arguments" in V.last_error(), kw
    torch.cuda.synchronize()
    got = buf.got()
    assert (got[0] == FIC_GUARD).all() and (got[1] == POISON).all() and (got[2] == LEVEL_POISON).all()
    # what is allowed: both ends of the gain's range, no d_level, the per-carrier rule with its own range of gains
    for kw in (dict(soft=(1, 2.0 ** -24)), dict(soft=(1, 65536.0)), dict(soft=(1, 64.0), level=None),
               dict(soft=(0, 2.0 ** -30), level=None)):
        assert calls(**kw) == (0, 0), kw
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        V.ofdm_demap_soft_dev(d_fft, shape, d_b, 2, 64.0, 2, d_fic=a["d_fic"])
    with pytest.raises(ValueError):
        V.ofdm_demap_soft_dev(d_fft, shape, d_b, SOFT_PER_SYMBOL, 64.0, 2, d_fic=a["d_fic"], d_level=a["d_level"][:5])
    with pytest.raises(ValueError):
        V.ofdm_demod_soft_dev(d_iq, shape, d_b, SOFT_PER_SYMBOL, 64.0, 2, d_tw, nfft, nsyms * nfft, d_fic=a["d_fic"],
                              d_level=a["d_level"].to(torch.float64))


# ---- end to end -----------------------------------------------------------------------------------------------------

def test_end_to_end_through_the_echo_channel(V, O, torch_cuda):
    """8 mode-I frames of FIC symbols (96 FIBs) through the two-path channel in the time domain, AWGN at 5 dB ->
    vit_ofdm_demod_soft_dev with the per-symbol rule -> vit_decode_fic_dev: the FIBs and CRC flags of the CPU chain on
    the model's bytes"""
    rng = np.random.default_rng(2800)
    shape = (2048, 1536, 4, 3, 1)  # the phase reference and the FIC's three symbols
    nfft, K, nsyms = shape[0], shape[1], shape[2]
    nframes, guard = 8, 504
    ss = nfft + guard
    bins = freq_bins_model(nfft)[1]
    fibs, tx = fic_bits(O, rng, nframes)
    z = transmit(tx, bins, shape, rng, carrier_gain=echo_channel())
    x = time_domain(z, guard)
    sigma = np.sqrt(nfft * 10.0 ** (-5.0 / 10.0) / 2.0)  # 5 dB per unit carrier: a bin of the FFT holds nfft times the carrier
    x = (x + sigma * (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape))) / nfft
    start = guard - 100  # inside the guard, behind the echo of 37 samples
    parts = np.stack([[x[t, start + l * ss:start + l * ss + nfft] for l in range(nsyms)] for t in range(nframes)]).astype(np.complex64)
    tw = tw_tables(V, nfft)
    fs = nsyms * ss
    starts = np.arange(nframes, dtype=np.int64) * fs
    d_iq = torch.from_numpy(place(parts, starts, ss, nframes * fs)).cuda()
    d_fic = torch.full((nframes * 9216,), FIC_GUARD, dtype=torch.uint8, device="cuda")
    d_lev = torch.zeros((nframes, nsyms - 1), dtype=torch.float32, device="cuda")
    V.ofdm_demod_soft_dev(d_iq, shape, dev_bins(bins), SOFT_PER_SYMBOL, 64.0, nframes, tw[1], ss, fs, d_fic=d_fic, d_level=d_lev)
    nblk = 4 * nframes
    d_fibs = torch.zeros((nblk, 96), dtype=torch.uint8, device="cuda")
    d_ok = torch.zeros((nblk * 3,), dtype=torch.uint8, device="cuda")
    V.decode_fic_dev(d_fic, d_fibs, d_ok, 768, nblk, fic_segments())
    torch.cuda.synchronize()
    out, S = demap_soft_model(Rotation(V, rng, nframes, 0).model(V, parts, ss), bins, shape, 64.0)
    assert np.array_equal(d_fic.cpu().numpy(), out.reshape(-1))
    assert np.array_equal(d_lev.cpu().numpy().view(np.uint32), S.view(np.uint32))
    want = fic_decode(O, out.reshape(-1, 2304))
    assert np.array_equal(d_fibs.cpu().numpy(), want)
    assert np.array_equal(d_ok.cpu().numpy(), fib_ok_model(want.reshape(-1, 32)).astype(np.uint8))
    good = d_ok.cpu().numpy().reshape(-1, 3).all(axis=1)  # coding blocks whose three CRCs hold: the FIBs sent
    assert good.mean() > 0.5 and np.array_equal(want[good], fibs[good])
