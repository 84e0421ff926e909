"""GPU: "Integer sample formats" - vit_iq_convert_dev bitwise against the numpy model of tests/test_iqfmt_host.py, and the
three *_iq_dev calls against the existing float32 models fed the converted floats (front_model by value, demap_model
byte-exact, sync_model in every output word) and against the existing calls fed the output of vit_iq_convert_dev, with
no model in the loop.  Every call runs twice, on two raw buffers that agree on exactly the samples the header says are
read and differ in every other byte, and must give the same outputs: integers have no NaN to poison with.  The raw
tensors start 4 bytes behind their allocation, so that CU8 samples sit at addresses that are 2 mod 4, and end with the
last read sample.  Then the skip rules, VIT_IQ_F32 through the new entries, the argument rules, and end to end from a
CU8 stream into vit_decode_fic_dev."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (torch's runtime first, as when the whole suite is collected)

from test_dab_host import fib_ok_model
from test_fft_host import LENGTHS, cfo_step, time_domain
from test_gpu_ofdm import FIC_GUARD, GUARD, ODD_SHAPES, POISON, dev_bins, subset_bins
from test_gpu_ofdm_td import GUARDS, Layout, Rotation, dev_u32, nco_tables, transmitted_parts, tw_tables
from test_gpu_sync import GW, SENT32, SENT64, SHAPES, directed
from test_iqfmt_host import DTYPES, INT_FORMATS, IQ_CS8, IQ_CS16, IQ_CU8, SCALES, USUAL_SCALE, all_codes, convert_model, quantise
from test_ofdm_host import MODE_III, demap_model, fic_bits, freq_bins_model, split_model
from test_punct_host import fic_segments
from test_sync_host import Params, prs_table, sync_model

pytestmark = pytest.mark.gpu

NAMES = {IQ_CU8: "cu8", IQ_CS8: "cs8", IQ_CS16: "cs16"}
fmt_param = pytest.mark.parametrize("fmt", INT_FORMATS, ids=[NAMES[f] for f in INT_FORMATS])


def random_codes(rng, fmt, shape):
    info = np.iinfo(DTYPES[fmt])
    return rng.integers(info.min, info.max + 1, tuple(shape) + (2,)).astype(DTYPES[fmt])


def extreme_codes(rng, fmt, shape):
    """full-range inputs, symbol by symbol (shape = (nframes, nsyms, nfft)): every component the smallest code, the
    largest, a random choice of the two, for CS16 -32767 against 32767, and - CS8 and CS16 - all-zero symbols"""
    info = np.iinfo(DTYPES[fmt])
    lo, hi = info.min, info.max
    out = np.empty(tuple(shape) + (2,), DTYPES[fmt])
    kinds = 4 if fmt == IQ_CU8 else 5
    for t in range(shape[0]):
        for l in range(shape[1]):
            kind = (t + l) % kinds
            pick = rng.integers(0, 2, (shape[2], 2)).astype(bool)
            out[t, l] = [np.where(pick, hi, lo), np.full_like(pick, lo, DTYPES[fmt]), np.full_like(pick, hi, DTYPES[fmt]),
                         np.where(pick, hi, -hi if lo < 0 else lo), np.zeros_like(pick, DTYPES[fmt])][kind]
    return out


def place_raw(parts, starts, sym_stride, background):
    """raw useful parts (nframes, nsyms, nfft, 2) at samples starts[t] + l*sym_stride of a copy of `background`
    (nsamples, 2) -> (buffer, mask of the samples that were placed)"""
    buf = background.copy()
    mask = np.zeros(buf.shape[0], bool)
    nfft = parts.shape[2]
    for t in range(parts.shape[0]):
        for l in range(parts.shape[1]):
            o = int(starts[t]) + l * sym_stride
            buf[o:o + nfft] = parts[t, l]
            mask[o:o + nfft] = True
    return buf, mask


def other_bytes(buf, mask):
    """the buffer with every byte of every sample outside `mask` changed"""
    return np.where(mask[:, None], buf, ~buf)


def dev_raw(buf):
    """(nsamples, 2) raw samples -> a CUDA tensor of exactly 2*nsamples elements that starts 4 bytes behind its allocation"""
    pad = 4 // buf.dtype.itemsize
    t = torch.empty(pad + buf.size, dtype=torch.from_numpy(buf[:1]).dtype, device="cuda")
    d = t[pad:]
    d.copy_(torch.from_numpy(np.ascontiguousarray(buf).reshape(-1)))
    assert d.data_ptr() % 8 == 4 and d.numel() == buf.size
    return d


def dev_floats(V, d_raw, fmt, scale):
    """the floats vit_iq_convert_dev makes of a raw tensor (complex64, one element per sample)"""
    d = torch.full((d_raw.numel() // 2,), complex(float("nan"), float("nan")), dtype=torch.complex64, device="cuda")
    V.iq_convert_dev(d_raw, fmt, scale, d)
    return d


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8).reshape(-1), b.contiguous().view(torch.uint8).reshape(-1))


# ---- 1. vit_iq_convert_dev ----------------------------------------------------------------------------------------------

@fmt_param
def test_convert_equals_the_model(V, torch_cuda, fmt):
    """every code of the format at five scales, and nsamples 0, 1, 3, 17 and 4099 (heads and tails of every 16-byte
    phase of the input, outputs on and off 16 bytes), into a guarded, poisoned output compared whole, bit for bit"""
    rng = np.random.default_rng(1100 + fmt)
    codes = all_codes(fmt)
    case = 0
    for scale in SCALES:
        for n in (codes.shape[0], 0, 1, 3, 17, 4099):
            raw = codes if n == codes.shape[0] else random_codes(rng, fmt, (n,))
            if 0 < n != codes.shape[0]:
                raw[:min(n, codes.shape[0])] = rng.permutation(codes)[:n]
            in_off, out_off = 4 * (case % 4) // raw.dtype.itemsize, 2 * (case // 4 % 2)  # elements: 0 ... 12 and 0 or 8 bytes
            case += 1
            d_in = torch.zeros(in_off + max(raw.size, 2), dtype=torch.from_numpy(raw[:1]).dtype, device="cuda")
            d_in[in_off:in_off + raw.size].copy_(torch.from_numpy(raw.reshape(-1)))
            out = torch.full((out_off + 2 * n + 8,), float("nan"), dtype=torch.float32, device="cuda")
            V.iq_convert_dev(d_in[in_off:], fmt, scale, out[out_off:], nsamples=n)
            torch.cuda.synchronize()
            want = np.full(out.numel(), np.nan, np.float32)
            want[out_off:out_off + 2 * n] = convert_model(raw, fmt, scale).view(np.float32).reshape(-1)
            assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)), (scale, n, in_off, out_off)


# ---- 2. vit_ofdm_fft_iq_dev ---------------------------------------------------------------------------------------------

def run_fft_iq(V, rng, fmt, scale, parts, lay, rot):
    nframes, nsyms, nfft = parts.shape[:3]
    buf, mask = place_raw(parts, lay.starts, lay.sym_stride, random_codes(rng, fmt, (lay.nsamples,)))
    want = rot.model(V, convert_model(parts, fmt, scale), lay.sym_stride)
    outs, d_raws = [], [dev_raw(buf), dev_raw(other_bytes(buf, mask))]
    for d_iq in d_raws:
        d_fft = torch.full((nframes * nsyms * nfft + 4,), complex(float("nan"), float("nan")), dtype=torch.complex64, device="cuda")
        V.ofdm_fft_dev(d_iq, nfft, nsyms, nframes, d_fft=d_fft, iq_format=fmt, iq_scale=scale, **lay.args(), **rot.args(V, nfft))
        outs.append(d_fft)
    d_flt = dev_floats(V, d_raws[0], fmt, scale)
    d_ref = torch.full_like(outs[0], complex(float("nan"), float("nan")))
    V.ofdm_fft_dev(d_flt, nfft, nsyms, nframes, d_fft=d_ref, **lay.args(), **rot.args(V, nfft))
    torch.cuda.synchronize()
    got = outs[0].cpu().numpy()
    g = got[:-4].reshape(nframes, nsyms, nfft)
    assert np.array_equal(g.real, want.real) and np.array_equal(g.imag, want.imag)  # by value: -0 == +0
    assert np.isnan(got[-4:].real).all()
    assert same_bits(outs[0], outs[1]), "a byte outside the useful parts influenced a spectrum"
    assert same_bits(outs[0], d_ref), "the float32 call on vit_iq_convert_dev's floats"


@fmt_param
@pytest.mark.parametrize("nfft", LENGTHS)
def test_fft_equals_the_model(V, torch_cuda, fmt, nfft):
    """every length, 3 frames of 3 symbols of random codes, without rotation and with it (the corner steps and random
    ones), frames by stride and by an out-of-order table of odd positions"""
    rng = np.random.default_rng(1200 + 16 * nfft + fmt)
    scale = USUAL_SCALE[fmt]
    for nco_bits, steps in ((0, None), (20, [0, 1 << 31, (1 << 32) - 1]), (10, [1, 12345, int(rng.integers(0, 1 << 32))])):
        for table in (False, True):
            run_fft_iq(V, rng, fmt, scale, random_codes(rng, fmt, (3, 3, nfft)), Layout(rng, 3, 3, nfft, table),
                       Rotation(V, rng, 3, nco_bits, steps))


# ---- 3. vit_ofdm_demod_iq_dev -------------------------------------------------------------------------------------------

def run_demod_iq(V, rng, fmt, scale, parts, bins, shape, gain, lay, rot, use_fic=True, use_ring=True, nrows=None, first_row=0,
                 col=0, extra=0, fic_offset=3, ring_offset=1, skipped=()):
    """the call on guarded, poisoned buffers at odd offsets, on the two raw buffers; the whole output buffers are compared
    with the model's image of them (the frames in `skipped` keep their poison) and with the float32 call's"""
    nfft, K, nsyms, fic_syms, cifs = shape
    nframes = parts.shape[0]
    per = (nsyms - 1 - fic_syms) // cifs
    keep = [t for t in range(nframes) if t not in skipped]
    buf, mask = place_raw(parts[keep], lay.starts[keep], lay.sym_stride, random_codes(rng, fmt, (lay.nsamples,)))
    nrows = nframes * cifs if nrows is None else nrows
    row_bytes = col + per * 2 * K + extra
    fic_n = nframes * fic_syms * 2 * K

    def call(d_iq, **fmt_args):
        fic_buf = torch.full((fic_offset + fic_n + GUARD,), FIC_GUARD, dtype=torch.uint8, device="cuda")
        ring_buf = torch.full((ring_offset + nrows * row_bytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        d_ring = ring_buf[ring_offset:ring_offset + nrows * row_bytes].view(nrows, row_bytes)
        V.ofdm_demod_dev(d_iq, shape, dev_bins(bins), gain, nframes, d_fic=fic_buf[fic_offset:] if use_fic else None,
                         d_ring=d_ring if use_ring else None, first_row=first_row, col=col, nsamples=lay.nsamples, **fmt_args,
                         **lay.args(), **rot.args(V, nfft))
        return fic_buf, ring_buf

    outs = [call(dev_raw(b), iq_format=fmt, iq_scale=scale) for b in (buf, other_bytes(buf, mask))]
    ref = call(dev_floats(V, dev_raw(buf), fmt, scale))
    torch.cuda.synchronize()
    want_fic = np.full(outs[0][0].numel(), FIC_GUARD, np.uint8)
    want_ring = np.full(outs[0][1].numel(), POISON, np.uint8)
    out = demap_model(rot.model(V, convert_model(parts, fmt, scale), lay.sym_stride), bins, shape, gain)
    mark = np.zeros_like(out)
    mark[keep] = 1  # a skipped frame's bytes stay as they were
    fic_img, ring_img = np.zeros(fic_n, np.uint8), np.zeros((nrows, row_bytes), np.uint8)
    fic_own, ring_own = np.zeros(fic_n, np.uint8), np.zeros((nrows, row_bytes), np.uint8)
    split_model(out, shape, fic=fic_img if use_fic else None, ring=ring_img if use_ring else None, first_row=first_row, col=col)
    split_model(mark, shape, fic=fic_own if use_fic else None, ring=ring_own if use_ring else None, first_row=first_row, col=col)
    want_fic[fic_offset:fic_offset + fic_n][fic_own == 1] = fic_img[fic_own == 1]
    want_ring[ring_offset:ring_offset + nrows * row_bytes].reshape(nrows, row_bytes)[ring_own == 1] = ring_img[ring_own == 1]
    assert np.array_equal(outs[0][0].cpu().numpy(), want_fic), "d_fic and its guards"
    assert np.array_equal(outs[0][1].cpu().numpy(), want_ring), "the ring, its poison and its guards"
    for other, what in ((outs[1], "a byte outside the useful parts influenced an output"), (ref, "the float32 call")):
        assert torch.equal(outs[0][0], other[0]) and torch.equal(outs[0][1], other[1]), what


@fmt_param
@pytest.mark.parametrize("shape,kind", ODD_SHAPES)
def test_demod_odd_shapes(V, torch_cuda, fmt, shape, kind):
    """K = 1, odd K, tables that are not the standard's, per = 1, no FIC symbols, no CIFs, nfft 64 ... 8192; random codes and
    the full-range inputs; d_fic only, ring only, both; with and without rotation, strides and a table"""
    rng = np.random.default_rng(1300 + shape[0] + shape[1] + fmt)
    nfft, K, nsyms, fic_syms, cifs = shape
    bins = freq_bins_model(nfft)[1] if kind == "std" else subset_bins(rng, nfft, K)
    for i, (nframes, use_fic, use_ring) in enumerate(((2, True, True), (5, False, True), (4, True, False))):
        parts = (random_codes, extreme_codes, random_codes)[i](rng, fmt, (nframes, nsyms, nfft))
        nrows = nframes * cifs + int(rng.integers(0, 20))
        run_demod_iq(V, rng, fmt, (USUAL_SCALE[fmt], 1.0, SCALES[4])[i], parts, bins, shape, float(rng.choice([1.0, 180.5, 254.0])),
                     Layout(rng, nframes, nsyms, nfft, bool(i & 1)), Rotation(V, rng, nframes, (10, 0, 20)[i]),
                     use_fic=use_fic, use_ring=use_ring, nrows=nrows, first_row=int(rng.integers(0, nrows)),
                     col=int(rng.integers(0, 40)), extra=int(rng.integers(1, 9)), fic_offset=int(rng.integers(0, 8)),
                     ring_offset=int(rng.integers(0, 8)))


@fmt_param
@pytest.mark.parametrize("nfft", sorted(GUARDS))
def test_demod_reduced_modes(V, torch_cuda, fmt, nfft):
    """one reduced frame per transmission mode - its length, carriers, guard and table, 6 symbols -: the transmitter's
    samples with noise and a frequency offset, rounded to the format, and the full-range inputs"""
    rng = np.random.default_rng(1400 + nfft + fmt)
    shape = (nfft, 3 * nfft // 4, 6, 2, 3)
    bins = freq_bins_model(nfft)[1]
    parts, ss = transmitted_parts(rng, bins, shape, 2, rng, cfo=0.3, snr_db=10.0)
    raw, scale = quantise(parts, fmt)
    run_demod_iq(V, rng, fmt, scale, raw, bins, shape, 254.0, Layout(rng, 2, 6, nfft, True, sym_stride=ss),
                 Rotation(V, rng, 2, 20, [cfo_step(0.3, nfft)] * 2), nrows=9, first_row=7, col=7, extra=4)
    run_demod_iq(V, rng, fmt, scale, extreme_codes(rng, fmt, (3, 6, nfft)), bins, shape, 254.0,
                 Layout(rng, 3, 6, nfft, False, sym_stride=ss), Rotation(V, rng, 3, 0))


# ---- 4. vit_ofdm_sync_iq_dev --------------------------------------------------------------------------------------------

def sync_reads(coarse, prm, n):
    """the samples the definition reads: the guard pairs of step A and the window of step B of every frame that is not skipped"""
    mask = np.zeros(n, bool)
    for c in (int(v) for v in coarse):
        if c - prm.W < 0 or c - prm.W + prm.span() > n:
            continue
        mask[c - prm.W:c - prm.W + prm.nfft] = True
        for l in range(1, prm.cp_symbols + 1):
            o = c + l * prm.sym_stride - prm.guard + prm.W
            mask[o:o + prm.guard - 2 * prm.W] = True
            mask[o + prm.nfft:o + prm.nfft + prm.guard - 2 * prm.W] = True
    return mask


def run_sync_iq(V, fmt, scale, raw, prm, prs, coarse, nframes, table=True, alias=False, nco_bits=12, frame_stride=None):
    """one call on guarded outputs, on the two raw buffers (exactly raw.shape[0] samples each); the whole output buffers are
    compared with the model's image on the converted floats and with the float32 call's"""
    nfft = prm.nfft
    tw, d_tw = tw_tables(V, nfft)
    nco, d_nco = nco_tables(V, nco_bits)
    d_prs = torch.from_numpy(prs).cuda()
    coarse = np.asarray(coarse[:nframes], np.int64)
    mask = sync_reads(coarse, prm, raw.shape[0])

    def call(d_iq, **fmt_args):
        so = torch.full((2 * GW + nframes,), SENT64, dtype=torch.int64, device="cuda")
        ro = dev_u32(np.full(2 * (2 * GW + nframes), SENT32, np.uint32))
        io = dev_u32(np.full(10 + 8 * nframes, SENT32, np.uint32))
        d_so = so[GW:GW + nframes]
        d_start = None
        if table:
            d_start = torch.from_numpy(coarse).cuda()
            if alias:
                d_so.copy_(d_start)
                d_start = d_so
        V.ofdm_sync_dev(d_iq, nfft, prm.nsyms, nframes, d_tw, prm.sym_stride, d_nco, nco_bits, d_prs, d_so, ro[2 * GW:], prm.W,
                        prm.M, cp_symbols=prm.cp_symbols, thr=prm.thr, backoff=prm.backoff, frame_stride=frame_stride,
                        first_start=0 if table else int(coarse[0]), d_start=d_start, d_info=io[5:], **fmt_args)
        return so, ro, io

    outs = [call(dev_raw(b), iq_format=fmt, iq_scale=scale) for b in (raw, other_bytes(raw, mask))]
    ref = call(dev_floats(V, dev_raw(raw), fmt, scale))
    torch.cuda.synchronize()
    start, rot, info, _ = sync_model(convert_model(raw, fmt, scale), coarse, prm, prs, tw, nco, nco_bits)
    so, ro, io = (t.cpu().numpy() for t in outs[0])
    want_so = np.full(so.size, SENT64, np.int64)
    want_so[GW:GW + nframes] = start
    want_ro = np.full(ro.size, SENT32, np.uint32)
    want_ro[2 * GW:2 * GW + 2 * nframes] = rot.reshape(-1)
    want_io = np.full(io.size, SENT32, np.uint32)
    want_io[5:5 + 8 * nframes] = info.reshape(-1)
    assert np.array_equal(so, want_so), "starts and their guards"
    assert np.array_equal(ro.view(np.uint32), want_ro), "rot and its guards"
    ints = np.zeros(io.size, bool)
    ints[5:5 + 8 * nframes] = np.tile(np.arange(8) < 2, nframes)
    assert np.array_equal(io.view(np.uint32)[ints], want_io[ints]), "m^ and tau"
    # the six floats by value (-0 = +0), everything else bit for bit
    assert np.array_equal(io.view(np.uint32)[~ints].view(np.float32), want_io[~ints].view(np.float32)), "info floats and the guards"
    for other, what in ((outs[1], "a byte outside the guard pairs and the window influenced an output"), (ref, "the float32 call")):
        assert all(same_bits(a, b) for a, b in zip(outs[0], other)), what
    return start


def quantised_directed(fmt, shape, nframes=8, uniform=False):
    x, true, coarse, prs = directed(shape, nframes, uniform)
    raw, scale = quantise(x, fmt)
    return raw, scale, true, coarse, prs


@pytest.mark.parametrize("fmt", (IQ_CS16, IQ_CU8, IQ_CS8), ids=("cs16", "cu8", "cs8"))
@pytest.mark.parametrize("shape", SHAPES)
def test_sync_equals_the_model(V, torch_cuda, fmt, shape):
    """the directed frames of tests/test_gpu_sync.py rounded to the format (CS16 at 2^-15, CU8 at 2^-8, CS8 at 2^-7): the
    coarse table, once aliased by the output, and first_start + stride with the buffer ending at the last frame's span"""
    nfft, G, nsyms, W, M = shape
    raw, scale, true, coarse, prs = quantised_directed(fmt, shape)
    assert scale == USUAL_SCALE[fmt]
    start = run_sync_iq(V, fmt, scale, raw, Params(nfft, G, nsyms, W, M, thr=0.5, backoff=3), prs, coarse, 8)
    assert (start != -1).all()
    run_sync_iq(V, fmt, scale, raw, Params(nfft, G, nsyms, W, M, cp_symbols=min(2, nsyms - 1)), prs, coarse[::-1].copy(), 3,
                alias=True, nco_bits=20)
    raw, scale, true, coarse, prs = quantised_directed(fmt, shape, 5, uniform=True)
    stride = int(true[1] - true[0])
    prm = Params(nfft, G, nsyms, W, M, cp_symbols=1, thr=1.0)
    for nframes in (1, 3):
        n = int(coarse[nframes - 1]) - W + prm.span()
        start = run_sync_iq(V, fmt, scale, raw[:n], prm, prs, coarse, nframes, table=False, frame_stride=stride)
        assert (start != -1).all()


# ---- 6. the skip rules ------------------------------------------------------------------------------------------------

@fmt_param
def test_skipped_frames(V, torch_cuda, fmt):
    """tables with starts of -1, far outside, past the end, a last read at nsamples (the last frame that fits) and at
    nsamples + 1: the demodulator's skipped frames keep every output byte, the sync's get -1, {0, 0} and zeros, and both
    agree with the float32 call on the same table"""
    rng = np.random.default_rng(1600 + fmt)
    shape = (128, 77, 9, 2, 3)
    nfft, K, nsyms, fic_syms, cifs = shape
    nframes = 7
    lay = Layout(rng, nframes, nsyms, nfft, True)
    extent = (nsyms - 1) * lay.sym_stride + nfft
    lay.starts = np.array([-1, 5, lay.nsamples - extent + 1, lay.nsamples - extent, -(1 << 62), lay.nsamples, 1 << 62], np.int64)
    lay.d_start = torch.from_numpy(lay.starts).cuda()
    run_demod_iq(V, rng, fmt, USUAL_SCALE[fmt], random_codes(rng, fmt, (nframes, nsyms, nfft)), subset_bins(rng, nfft, K), shape,
                 254.0, lay, Rotation(V, rng, nframes, 10), nrows=nframes * cifs + 2, first_row=3, col=1, extra=2,
                 skipped=(0, 2, 4, 5, 6))
    sshape = SHAPES[1]
    nfft, G, nsyms, W, M = sshape
    raw, scale, true, coarse, prs = quantised_directed(fmt, sshape)
    prm = Params(nfft, G, nsyms, W, M)
    n = raw.shape[0] - 7
    last = n - prm.span() + W  # the last coarse start whose span is inside
    table = np.array([W - 1, W, -1, last + 1, last, -(1 << 62), 1 << 62, n, int(coarse[1])], np.int64)
    for alias in (False, True):
        start = run_sync_iq(V, fmt, scale, raw[:n], prm, prs, table, table.size, alias=alias)
        assert ((start == -1) == np.array([1, 0, 1, 1, 0, 1, 1, 1, 0], bool)).all()


# ---- 7. VIT_IQ_F32 through the new entries ------------------------------------------------------------------------------

def test_f32_through_the_iq_entries(V, torch_cuda):
    """format VIT_IQ_F32 is the existing call, bit for bit; its scale - NaN here - is ignored"""
    L = V.lib()
    rng = np.random.default_rng(1700)
    f32 = C.byref(V.IqFormat(V.IQ_F32, float("nan")))
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    shape = (512, 384, 6, 2, 3)
    nfft, K, nsyms, fic_syms, cifs = shape
    nframes = 3
    lay, rot = Layout(rng, nframes, nsyms, nfft, True), Rotation(V, rng, nframes, 20)
    x = (rng.standard_normal(lay.nsamples) + 1j * rng.standard_normal(lay.nsamples)).astype(np.complex64)
    d_iq = torch.from_numpy(x).cuda()
    d_b = dev_bins(freq_bins_model(nfft)[1])
    inp = V.iq_input(d_iq, nsamples=lay.nsamples, **lay.args(), **rot.args(V, nfft))
    a = [torch.full((nframes, nsyms, nfft), complex(float("nan"), 0.0), dtype=torch.complex64, device="cuda") for _ in range(2)]
    assert L.vit_ofdm_fft_dev(C.byref(inp), nfft, nsyms, nframes, P(a[0]), nfft, nsyms * nfft, s) == 0
    assert L.vit_ofdm_fft_iq_dev(C.byref(inp), f32, nfft, nsyms, nframes, P(a[1]), nfft, nsyms * nfft, s) == 0
    fic = [torch.full((nframes * fic_syms * 2 * K,), FIC_GUARD, dtype=torch.uint8, device="cuda") for _ in range(2)]
    ring = [torch.full((nframes * cifs, 2 * K), POISON, dtype=torch.uint8, device="cuda") for _ in range(2)]
    sh = C.byref(V.OfdmShape(*shape))
    assert L.vit_ofdm_demod_dev(C.byref(inp), P(d_b), sh, 254.0, nframes, P(fic[0]), C.byref(V.cif_ring(ring[0], 0)), 0, s) == 0
    assert L.vit_ofdm_demod_iq_dev(C.byref(inp), f32, P(d_b), sh, 254.0, nframes, P(fic[1]), C.byref(V.cif_ring(ring[1], 0)), 0, s) == 0
    torch.cuda.synchronize()
    assert same_bits(a[0], a[1]) and not bool(torch.isnan(a[0].real).any())
    assert torch.equal(fic[0], fic[1]) and torch.equal(ring[0], ring[1]) and bool((ring[0] != POISON).any())
    nfft, G, nsyms, W, M = SHAPES[1]
    x, true, coarse, prs = directed(SHAPES[1])
    prm = Params(nfft, G, nsyms, W, M)
    d_x, d_prs, d_c = torch.from_numpy(x).cuda(), torch.from_numpy(prs).cuda(), torch.from_numpy(coarse).cuda()
    inp = V.iq_input(d_x, tw_tables(V, nfft)[1], prm.sym_stride, 0, d_c, nco_tables(V, 12)[1], 12)
    par = C.byref(V.SyncParams(nfft, nsyms, nsyms - 1, W, M, 0.5, 0, 0))
    outs = [(torch.zeros(8, dtype=torch.int64, device="cuda"), torch.zeros(16, dtype=torch.int32, device="cuda"),
             torch.zeros(64, dtype=torch.int32, device="cuda")) for _ in range(2)]
    assert L.vit_ofdm_sync_dev(C.byref(inp), par, P(d_prs), 8, P(outs[0][0]), P(outs[0][1]), P(outs[0][2]), s) == 0
    assert L.vit_ofdm_sync_iq_dev(C.byref(inp), f32, par, P(d_prs), 8, P(outs[1][0]), P(outs[1][1]), P(outs[1][2]), s) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(*outs)) and bool((outs[0][0] > 0).any()) and bool((outs[0][2] != 0).any())


# ---- the argument rules -------------------------------------------------------------------------------------------------

def test_argument_errors(V, torch_cuda):
    """the rules the formats add are VIT_ERR_ARG with a message and launch nothing: the scale's range, d_iq 4-byte aligned for
    the integer formats and 8-byte aligned for VIT_IQ_F32, vit_iq_convert_dev's own; what is allowed is VIT_OK"""
    L = V.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nfft, nsyms, ss = 64, 2, 80
    d_raw = torch.zeros(4 * (ss + nfft) + 16, dtype=torch.uint8, device="cuda")
    d_tw = tw_tables(V, nfft)[1]
    d_fft = torch.full((nsyms * nfft,), 3.0 + 0j, dtype=torch.complex64, device="cuda")
    d_out = torch.full((64,), 3.0, dtype=torch.float32, device="cuda")

    def fft(fmt, scale, off, nsamples=ss + nfft):
        inp = V.iq_input(d_raw, d_tw, ss, 0, nsamples=nsamples, iq_format=V.IQ_CU8)
        inp.d_iq = d_raw.data_ptr() + off
        return L.vit_ofdm_fft_iq_dev(C.byref(inp), C.byref(V.IqFormat(fmt, scale)), nfft, nsyms, 1, C.c_void_p(d_fft.data_ptr()),
                                     nfft, nsyms * nfft, s)

    def convert(fmt, scale, in_off=0, out_off=0, n=8, null=False):
        return L.vit_iq_convert_dev(None if null else C.c_void_p(d_raw.data_ptr() + in_off), C.byref(V.IqFormat(fmt, scale)), n,
                                    C.c_void_p(d_out.data_ptr() + out_off), s)

    bad = [fft(V.IQ_CU8, 1.0, 2), fft(V.IQ_CS8, 1.0, 1), fft(V.IQ_CS16, 1.0, 2), fft(V.IQ_F32, 1.0, 4), fft(V.IQ_CU8, 2.0 ** 17, 0),
           fft(V.IQ_CS16, 2.0 ** -33, 0), fft(V.IQ_CS8, float("nan"), 0), fft(V.IQ_CS8, 0.0, 0), fft(7, 1.0, 0),
           fft(V.IQ_CU8, 1.0, 0, nsamples=ss + nfft - 1),
           convert(V.IQ_F32, 1.0), convert(V.IQ_CU8, 1.0, in_off=2), convert(V.IQ_CS16, 1.0, out_off=4), convert(V.IQ_CS8, 2.0 ** 17),
           convert(V.IQ_CU8, 1.0, null=True), convert(4, 1.0)]
    assert bad == [1] * len(bad)
    assert "bad arguments" in V.last_error()
    assert convert(V.IQ_CU8, 1.0, n=0) == 0
    torch.cuda.synchronize()
    assert bool((d_fft == 3.0).all()) and bool((d_out == 3.0).all())
    assert fft(V.IQ_CU8, 2.0 ** -32, 4) == 0 and fft(V.IQ_CS8, 2.0 ** 16, 12) == 0 and fft(V.IQ_CS16, 1.0, 4, nsamples=ss + nfft) == 0
    assert convert(V.IQ_CS16, 1.0, in_off=12, out_off=8) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        V.ofdm_fft_dev(d_raw, nfft, nsyms, 1, d_tw, ss, d_fft, frame_stride=0, iq_format=V.IQ_CS16)  # uint8 is not int16
    with pytest.raises(ValueError):
        V.ofdm_fft_dev(d_raw, nfft, nsyms, 1, d_tw, ss, d_fft, frame_stride=0)  # nor float32
    with pytest.raises(ValueError):
        V.iq_convert_dev(d_raw, V.IQ_F32, 1.0, d_out)
    with pytest.raises(ValueError):
        V.iq_convert_dev(d_raw, V.IQ_CU8, 1.0, d_out)  # d_out is too small


# ---- 8. end to end --------------------------------------------------------------------------------------------------

def transmit_bits(prm, prs, bins, bits, offsets, lead):
    """the transmitter of tests/test_sync_host.py (transmit_frames) for given bits (nframes, nsyms-1, 2K), noise-free: the
    known reference symbol, DQPSK data, a frequency offset of offsets[t] carrier spacings and lead[t] samples of silence
    per frame -> (samples complex128, true starts)"""
    nfft, G, K = prm.nfft, prm.guard, len(bins)
    nframes = bits.shape[0]
    q = ((1 - 2 * bits[:, :, :K]) + 1j * (1 - 2 * bits[:, :, K:])) / np.sqrt(2.0)
    ref = np.broadcast_to(np.asarray(prs, np.complex128)[np.asarray(bins, np.int64)], (nframes, 1, K))
    z = np.zeros((nframes, prm.nsyms, nfft), np.complex128)
    z[:, :, np.asarray(bins, np.int64)] = np.concatenate([ref, q], axis=1).cumprod(axis=1)
    chunks, starts, pos = [], [], 0
    for t in range(nframes):
        f = time_domain(z[t:t + 1], G, offsets[t])[0]
        chunks += [np.zeros(lead[t]), f, np.zeros(2 * prm.W + 2)]
        starts.append(pos + lead[t] + G)
        pos += lead[t] + f.size + 2 * prm.W + 2
    return np.concatenate(chunks), np.array(starts, np.int64)


def test_end_to_end_from_a_cu8_stream(V, O, torch_cuda):
    """no model in the loop: 3 noise-free mode-III frames that carry 4 FIC coding blocks (12 FIBs), with a start, an integer
    and a fractional carrier offset per frame, rounded to CU8 at 90 % of full range -> ofdm_sync_dev(CU8) writes the two
    tables -> ofdm_demod_dev(CU8) reads them -> vit_decode_fic_dev: every FIB CRC holds and the FIBs are the ones sent"""
    nfft, K, nsyms, fic_syms, cifs = MODE_III
    G, W, M, nframes, nco_bits = 63, 12, 6, 3, 12
    rng = np.random.default_rng(1800)
    prm = Params(nfft, G, nsyms, W, M, cp_symbols=20, thr=0.5, backoff=G // 2)
    bins = freq_bins_model(nfft)[1]
    prs = prs_table(rng, nfft, bins)
    fibs, fic_tx = fic_bits(O, rng, 1)  # one mode-I frame's FIC: 9216 bits, three mode-III frames' worth
    bits = rng.integers(0, 2, (nframes, nsyms - 1, 2 * K))
    bits[:, :fic_syms] = fic_tx.reshape(nframes, fic_syms, 2 * K)
    x, true = transmit_bits(prm, prs, bins, bits, [-5.5, 3.25, 0.49], [2 * W + 2 + int(v) for v in rng.integers(0, 50, nframes)])
    raw, scale = quantise(x, IQ_CU8)
    coarse = true + np.array([W, -W, 3])
    d_iq = dev_raw(raw)
    d_tw, d_nco = tw_tables(V, nfft)[1], nco_tables(V, nco_bits)[1]
    d_start = torch.from_numpy(coarse).cuda()
    d_rot = dev_u32(np.zeros((nframes, 2), np.uint32))
    V.ofdm_sync_dev(d_iq, nfft, nsyms, nframes, d_tw, prm.sym_stride, d_nco, nco_bits, torch.from_numpy(prs).cuda(), d_start,
                    d_rot, W, M, cp_symbols=prm.cp_symbols, thr=prm.thr, backoff=prm.backoff, d_start=d_start,
                    iq_format=V.IQ_CU8, iq_scale=scale)
    d_fic = torch.full((nframes, fic_syms * 2 * K), 128, dtype=torch.uint8, device="cuda")
    V.ofdm_demod_dev(d_iq, MODE_III, dev_bins(bins), 254.0, nframes, d_tw, prm.sym_stride, d_start=d_start, d_nco=d_nco,
                     nco_bits=nco_bits, d_rot=d_rot, d_fic=d_fic, iq_format=V.IQ_CU8, iq_scale=scale)
    d_fibs = torch.zeros((4, 96), dtype=torch.uint8, device="cuda")
    d_ok = torch.zeros((12,), dtype=torch.uint8, device="cuda")
    V.decode_fic_dev(d_fic, d_fibs, d_ok, 768, 4, fic_segments())
    torch.cuda.synchronize()
    assert bool((d_ok == 1).all())
    got = d_fibs.cpu().numpy()
    assert fib_ok_model(got.reshape(-1, 32)).all() and np.array_equal(got, fibs)
