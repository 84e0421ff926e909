"""GPU: "Transmitter identification" - vit_ofdm_tii_dev against the numpy float32 model of tests/test_tii_host.py in every
output word (d_tii and d_energy), in guarded buffers compared whole: the transform lengths at which the FFT has another
pass structure (m mod 3 = 0, 1, 2) and the one with idle threads, frame counts 1, 7 and 19 with navg 1, 3 and 8 (a ragged
last group, a group per frame), odd and even sample positions, the four sample formats (a CU8 window at an address that is
2 mod 4), with and without d_rot, with the start table and with the stride, skipped frames, a group with nused 0,
all-zero windows, d_energy absent, the clamped table entry, the argument rules, the chain behind vit_ofdm_sync_dev, and
the independence of a group's words from nframes."""
import numpy as np
import pytest
import torch  # noqa: F401  (torch's runtime first, as when the whole suite is collected)

from test_gpu_iqfmt import dev_raw
from test_gpu_ofdm import dev_bins
from test_gpu_ofdm_td import dev_u32, nco_tables, tw_tables
from test_iqfmt_host import INT_FORMATS, IQ_CS8, IQ_CS16, IQ_CU8, quantise
from test_sync_host import Params, sync_model
from test_tii_host import (Tii, argument_error_cases, expected_masks, mask_of_main_id, masks_of, pair_bins_model, random_pairs,
                           tii_model, tii_stream)

pytestmark = pytest.mark.gpu

IQ_F32 = 0
FORMATS = (IQ_F32,) + INT_FORMATS
SENT32 = 0x5A5A5A5A
GW = 3  # guard words around both outputs
NCO_BITS = 12
# (nfft, Gp, C, R): m mod 3 = 0 with idle threads in the slot stage's workgroup, m mod 3 = 2, 0 and 2 again with 1, 1, 1
# and 3 slots for some threads
SHAPES = [(64, 4, 3, 2), (256, 8, 3, 4), (512, 8, 6, 2), (2048, 8, 24, 4)]
# the other four lengths, so that every instantiation the launcher can choose runs: small geometries and few frames (the
# model's time); 8192 is the one launch of this call that needs more than 64 KiB of dynamic LDS
OTHER_SHAPES = [(128, 2, 3, 2), (1024, 4, 5, 2), (4096, 8, 6, 2), (8192, 8, 24, 4)]
_cache = {}


def table_of(shape):
    nfft, Gp, C_, R = shape
    if shape not in _cache:
        _cache[shape] = pair_bins_model() if nfft == 2048 else random_pairs(np.random.default_rng(nfft), nfft, Gp, C_, R)
    return _cache[shape]


def make_case(shape, nframes=19):
    """Gaussian samples of unit power; in every frame's window the pairs of a few (mask, c) stand 10 dB and more above
    the noise of a bin.  The windows lie at odd and even positions, 3 ... 40 samples apart -> (x complex128, starts
    int64, offset), built once"""
    key = ("case", shape, nframes)
    if key not in _cache:
        nfft, Gp, C_, R = shape
        rng = np.random.default_rng(900 + nfft + nframes)
        pairs = table_of(shape).astype(np.int64)
        offset = -(nfft + 13)
        gaps = rng.integers(3, 41, nframes)
        w0 = np.cumsum(gaps + nfft) - nfft  # the windows' first samples
        assert (w0 % 2 == 0).any() and (w0 % 2 == 1).any()
        n = int(w0[-1]) + nfft + 5
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5)
        for t in range(nframes):
            Z = np.zeros(nfft, np.complex128)
            for c in rng.permutation(C_)[:2]:
                for b in np.flatnonzero(rng.integers(0, 2, Gp)):
                    k = pairs[:, b, c]
                    Z[k] = rng.uniform(3, 6) * np.sqrt(nfft) * np.exp(2j * np.pi * rng.random(R))
                    Z[k + 1] = rng.uniform(3, 6) * np.sqrt(nfft) * np.exp(2j * np.pi * rng.random(R))
            x[w0[t]:w0[t] + nfft] += np.fft.ifft(Z)
        _cache[key] = (x, (w0 - offset).astype(np.int64), offset)
    return _cache[key]


def in_format(x, fmt):
    """-> (what the device gets and the model reads: complex64 (n,) or raw (n, 2), the model's fmt argument)"""
    if fmt == IQ_F32:
        return np.asarray(x, np.complex64), None
    raw, scale = quantise(x, fmt)
    return raw, (fmt, scale)


def rot_table(rng, nframes):
    """any phase0 and steps of a few carrier spacings either way (small and near 2^32)"""
    rot = rng.integers(0, 1 << 32, (nframes, 2), dtype=np.uint64)
    rot[:, 1] = (rng.integers(-(1 << 23), 1 << 23, nframes) % (1 << 32)).astype(np.uint64)
    return rot.astype(np.uint32)


def run_tii(V, samples, mfmt, p, pairs, nframes, starts=None, frame_stride=None, rot=None, with_energy=True, nsamples=None,
            stream=None):
    """one call on guarded outputs; the whole buffers are compared with the model's image, bit for bit -> the model's
    (words, energy)"""
    n = len(samples) if nsamples is None else nsamples
    mstarts = np.arange(nframes) * frame_stride if starts is None else np.asarray(starts[:nframes])
    tw_h, d_tw = tw_tables(V, p.nfft)
    nco_h, d_nco = nco_tables(V, NCO_BITS)
    words, energy = tii_model(samples, mstarts, p, pairs, tw_h, nco_h, NCO_BITS, None if rot is None else rot[:nframes], mfmt, n)
    fmt, scale = (IQ_F32, 1.0) if mfmt is None else mfmt
    d_iq = torch.from_numpy(np.ascontiguousarray(samples)).cuda() if mfmt is None else dev_raw(samples)
    d_pairs = dev_bins(np.asarray(pairs).reshape(-1))
    to = dev_u32(np.full(2 * GW + words.size, SENT32, np.uint32))
    eo = dev_u32(np.full(2 * GW + energy.size, SENT32, np.uint32)).view(torch.float32)
    V.ofdm_tii_dev(d_iq, p.nfft, nframes, d_tw, d_pairs, to[GW:], p.Gp, p.C, p.R, p.navg, p.thr, p.offset,
                   d_start=None if starts is None else torch.from_numpy(np.asarray(starts, np.int64)).cuda(),
                   frame_stride=frame_stride, d_nco=None if rot is None else d_nco, nco_bits=0 if rot is None else NCO_BITS,
                   d_rot=None if rot is None else dev_u32(rot), d_energy=eo[GW:GW + energy.size] if with_energy else None,
                   nsamples=n, stream=stream, iq_format=fmt, iq_scale=scale)
    torch.cuda.synchronize()
    want_t = np.full(to.numel(), SENT32, np.uint32)
    want_t[GW:GW + words.size] = words.reshape(-1)
    want_e = np.full(eo.numel(), SENT32, np.uint32)
    if with_energy:
        want_e[GW:GW + energy.size] = energy.reshape(-1).view(np.uint32)
    assert np.array_equal(eo.cpu().numpy().view(np.uint32), want_e), "group energies and their guards"
    assert np.array_equal(to.cpu().numpy().view(np.uint32), want_t), "d_tii words and their guards"
    return words, energy


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: str(s[0]))
def test_shapes_against_the_model(V, torch_cuda, shape):
    """every format at frame counts 1, 7 and 19 with navg 1, 3 and 8, with and without d_rot and d_energy, windows at odd
    and even positions through the start table; the masks are not trivial"""
    nfft, Gp, C_, R = shape
    x, starts, offset = make_case(shape)
    pairs = table_of(shape)
    rot = rot_table(np.random.default_rng(nfft), 19)
    bits = 0
    for fmt in FORMATS:
        samples, mfmt = in_format(x, fmt)
        if fmt in (IQ_CU8, IQ_CS8):
            assert ((starts + offset) % 2 == 1).any()  # behind dev_raw's 4 bytes: a window at an address that is 2 mod 4
        combos = [(1, 1), (7, 3), (19, 8), (19, 1)] if fmt in (IQ_F32, IQ_CU8) else [(7, 8), (19, 3), (1, 8)]
        for i, (nframes, navg) in enumerate(combos):
            p = Tii(nfft, Gp, C_, R, navg=navg, thr=2.5, offset=offset)
            with_rot = (i + fmt) % 2 == 0
            words, _ = run_tii(V, samples, mfmt, p, pairs, nframes, starts=starts, rot=rot if with_rot else None,
                               with_energy=i % 2 == 0)
            assert (words[:-1, 0] == navg).all() and words[-1, 0] == nframes - (len(words) - 1) * navg
            bits += int(masks_of(words).astype(bool).sum())
    assert bits > 20


@pytest.mark.parametrize("shape", OTHER_SHAPES, ids=lambda s: str(s[0]))
def test_other_lengths_against_the_model(V, torch_cuda, shape):
    """float32 and CS16 at 3 and 2 frames with navg 2, 1 and 3 (a ragged last group, a group per frame), with and without
    d_rot and d_energy, windows at odd and even positions through the start table; the masks are not trivial"""
    nfft, Gp, C_, R = shape
    x, starts, offset = make_case(shape, nframes=3)
    pairs = table_of(shape)
    rot = rot_table(np.random.default_rng(nfft), 3)
    bits = 0
    for fmt, combos in ((IQ_F32, [(3, 2), (3, 1)]), (IQ_CS16, [(2, 3), (3, 2)])):
        samples, mfmt = in_format(x, fmt)
        for i, (nframes, navg) in enumerate(combos):
            p = Tii(nfft, Gp, C_, R, navg=navg, thr=2.5, offset=offset)
            words, _ = run_tii(V, samples, mfmt, p, pairs, nframes, starts=starts, rot=rot if i == 0 else None,
                               with_energy=(i + fmt) % 2 == 0)
            assert (words[:-1, 0] == navg).all() and words[-1, 0] == nframes - (len(words) - 1) * navg
            bits += int(masks_of(words).astype(bool).sum())
    assert bits > 4


@pytest.mark.parametrize("shape", (SHAPES[0], SHAPES[3]), ids=lambda s: str(s[0]))
def test_stride_layout(V, torch_cuda, shape):
    """no start table: frame t at t*frame_stride (odd), the window offset samples behind it, the buffer ending with the
    last window; float32, and CU8 with windows at addresses that are 2 mod 4"""
    nfft, Gp, C_, R = shape
    x = make_case(shape)[0]
    pairs = table_of(shape)
    stride, offset, nframes = nfft + 7, 5, 7
    n = (nframes - 1) * stride + offset + nfft
    rot = rot_table(np.random.default_rng(7), nframes)
    for fmt in (IQ_F32, IQ_CU8):
        samples, mfmt = in_format(x[:n + 9], fmt)
        p = Tii(nfft, Gp, C_, R, navg=3, thr=2.0, offset=offset)
        words, _ = run_tii(V, samples, mfmt, p, pairs, nframes, frame_stride=stride, rot=rot, nsamples=n)
        assert words[:, 0].tolist() == [3, 3, 1]
        run_tii(V, samples, mfmt, p, pairs, 2, frame_stride=stride, with_energy=False, nsamples=stride + offset + nfft)


def test_skipped_frames_and_empty_groups(V, torch_cuda):
    """start -1 and windows cut by either end of the buffer at both ends and in the middle of a group, a group with
    nused 0 between two that count, samples behind nsamples that must not be read (NaN, and the codes' complements)"""
    shape = SHAPES[1]
    nfft, Gp, C_, R = shape
    x, starts, offset = make_case(shape)
    pairs = table_of(shape)
    n = int(starts[-1]) + offset + nfft  # the buffer ends with the last window
    s = starts.copy()
    s[0] = -offset - 1       # group 0: cut in front | whole | -1 | whole
    s[2] = -1
    s[4:8] = [-1, n - offset - nfft + 1, -5, 2 ** 62]  # group 1: nothing counts
    s[8] = -1                # group 2: -1 | whole | whole | cut behind
    s[11] = n - offset - nfft + 1
    s[18] = n - offset - nfft  # the last window ends with the buffer
    for fmt in (IQ_F32, IQ_CS16, IQ_CU8):
        samples, mfmt = in_format(x, fmt)
        samples = samples.copy()
        if fmt == IQ_F32:
            samples[n:] = complex(np.nan, np.nan)
        else:
            samples[n:] = ~samples[n:]
        p = Tii(nfft, Gp, C_, R, navg=4, thr=2.5, offset=offset)
        words, energy = run_tii(V, samples, mfmt, p, pairs, 19, starts=s, rot=rot_table(np.random.default_rng(3), 19), nsamples=n)
        assert words[:, 0].tolist() == [2, 0, 2, 4, 3] and not words[1].any() and not energy[1].any() and energy[0].all()


def test_all_zero_windows(V, torch_cuda):
    """inside the domain: noise 0, every mask and strength 0, nused counts the frames; CS8 zeros and float zeros of both signs"""
    shape = SHAPES[2]
    nfft, Gp, C_, R = shape
    pairs = table_of(shape)
    p = Tii(nfft, Gp, C_, R, navg=2, thr=2.5, offset=-3)
    starts = np.array([3, 600, 1201], np.int64)
    z = np.zeros(1201 - 3 + nfft, np.complex64)
    z[1::2] = -z[1::2]
    raw = np.zeros((z.size, 2), np.int8)
    for samples, mfmt in ((z, None), (raw, (IQ_CS8, 2.0 ** -7))):
        words, energy = run_tii(V, samples, mfmt, p, pairs, 3, starts=starts, rot=rot_table(np.random.default_rng(5), 3))
        assert words[:, 0].tolist() == [2, 1] and not words[:, 1:].any() and not energy.any()


def test_clamped_table_entry_and_no_energy(V, torch_cuda):
    """an entry nfft-1 reads bins nfft-2 and nfft-1 as the entry nfft-2 does, at the first and the last length"""
    for shape in (SHAPES[0], SHAPES[3]):
        nfft, Gp, C_, R = shape
        x, starts, offset = make_case(shape)
        q = table_of(shape).copy()
        q[R - 1, Gp - 1, 1] = nfft - 1
        r = q.copy()
        r[R - 1, Gp - 1, 1] = nfft - 2
        p = Tii(nfft, Gp, C_, R, navg=2, thr=2.5, offset=offset)
        samples, mfmt = in_format(x, IQ_F32)
        a = run_tii(V, samples, mfmt, p, q, 4, starts=starts)
        b = run_tii(V, samples, mfmt, p, r, 4, starts=starts, with_energy=False)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_argument_errors(V, torch_cuda):
    assert argument_error_cases(V, torch) >= 40


def test_chain_behind_the_synchroniser(V, torch_cuda):
    """frames with a carrier offset of about 3 spacings: vit_ofdm_sync_dev writes d_start and d_rot, vit_ofdm_tii_dev reads
    them on the same stream with no synchronisation in between, and returns the transmitted (p, c) set through
    tii_main_id; every word equals the model behind sync_model"""
    nfft, G = 256, 64
    prm = Params(nfft, G, 4, 6, 4, backoff=5)
    p = Tii(nfft, 8, 3, 4, navg=4, thr=2.5, offset=-prm.sym_stride)
    rng = np.random.default_rng(300)
    pairs = random_pairs(rng, nfft, 8, 3, 4)
    sent = {(12, 0), (40, 2)}
    txs = [(mask_of_main_id(pid), c) for pid, c in sorted(sent)]
    x, true, prs = tii_stream(rng, prm, p, pairs, txs, 4, snr_db=20.0, tii_db=10.0, offsets=[3.0, 3.2, 2.7, 3.0])
    (tw_h, d_tw), (nco_h, d_nco) = tw_tables(V, nfft), nco_tables(V, NCO_BITS)
    start, rot, _, _ = sync_model(x, true - 3, prm, prs, tw_h, nco_h, NCO_BITS)
    words, energy = tii_model(x, start, p, pairs, tw_h, nco_h, NCO_BITS, rot)
    assert np.array_equal(masks_of(words)[0], expected_masks(p, txs))
    d_iq = torch.from_numpy(x).cuda()
    d_start = torch.from_numpy(true - 3).cuda()
    d_rot = dev_u32(np.full((4, 2), SENT32, np.uint32))
    d_tii = dev_u32(np.full(2 + 2 * p.C, SENT32, np.uint32))
    d_en = torch.full((p.Gp * p.C,), -1.0, dtype=torch.float32, device="cuda")
    d_prs, d_pairs = torch.from_numpy(prs).cuda(), dev_bins(pairs.reshape(-1))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        V.ofdm_sync_dev(d_iq, nfft, prm.nsyms, 4, d_tw, prm.sym_stride, d_nco, NCO_BITS, d_prs, d_start, d_rot, prm.W, prm.M,
                        thr=prm.thr, backoff=prm.backoff, d_start=d_start)
        V.ofdm_tii_dev(d_iq, nfft, 4, d_tw, d_pairs, d_tii, p.Gp, p.C, p.R, p.navg, p.thr, p.offset, d_start=d_start, d_nco=d_nco,
                       nco_bits=NCO_BITS, d_rot=d_rot, d_energy=d_en)
    side.synchronize()
    assert np.array_equal(d_start.cpu().numpy(), start) and np.array_equal(d_rot.cpu().numpy().view(np.uint32), rot)
    got = d_tii.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, words[0]) and np.array_equal(d_en.cpu().numpy().view(np.uint32), energy.reshape(-1).view(np.uint32))
    rec = V.tii_records(got, p.C)[0]
    found = {(V.tii_main_id(int(m)), c) for c, m in enumerate(rec["comb"]["mask"]) if m}
    assert rec["nused"] == 4 and found == sent


def test_a_group_does_not_depend_on_nframes(V, torch_cuda):
    """two calls on one buffer, 19 frames and 8: the groups both hold whole have the same words"""
    shape = SHAPES[3]
    nfft, Gp, C_, R = shape
    x, starts, offset = make_case(shape)
    pairs = table_of(shape)
    samples, mfmt = in_format(x, IQ_CS16)
    rot = rot_table(np.random.default_rng(11), 19)
    p = Tii(nfft, Gp, C_, R, navg=4, thr=2.5, offset=offset)
    w19, e19 = run_tii(V, samples, mfmt, p, pairs, 19, starts=starts, rot=rot)
    w8, e8 = run_tii(V, samples, mfmt, p, pairs, 8, starts=starts, rot=rot)
    assert w8.shape[0] == 2 and np.array_equal(w19[:2], w8) and np.array_equal(e19[:2].view(np.uint32), e8.view(np.uint32))
