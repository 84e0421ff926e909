"""GPU: "From the coarse start" - vit_ofdm_sync_dev against the numpy float32 model of tests/test_sync_host.py in every
output word (start, rot and the 8 info words), in guarded buffers compared whole: frames directed at the edges of the
search (m = -M and +M, tau = 0 and 2W, a fractional offset near +-1/2, odd sample positions, all-zero samples), frame
counts 1, 3 and 70, cp_symbols 1 and nsyms-1, W = 0 and M = 0, the coarse table and the stride, the output aliasing the
table, skipped frames at both ends of the buffer, the argument rules, and end to end into vit_ofdm_demod_dev."""
import numpy as np
import pytest
import torch  # noqa: F401  (torch's runtime first, as when the whole suite is collected)

from test_gpu_ofdm import dev_bins
from test_gpu_ofdm_td import dev_u32, nco_tables, tw_tables
from test_ofdm_host import MODE_III, freq_bins_model
from test_sync_host import Params, argument_error_cases, prs_table, std_bins, sync_model, transmit_frames

pytestmark = pytest.mark.gpu

SENT64, SENT32 = -0x0123456789ABCDEF, 0x5A5A5A5A
GW = 3  # guard entries around every output table (the info table's guard is 5 words: it is only 4-byte aligned)
# (nfft, guard, nsyms, W, M): the first three are the issue's; 256 has an odd G - 2W, so an accumulator tail
SHAPES = [(64, 16, 4, 4, 3), (256, 63, 8, 15, 8), (2048, 504, 6, 100, 16), (512, 126, 5, 30, 5), (1024, 252, 4, 61, 12)]
_cache = {}


def directed(shape, nframes=8, uniform=False):
    """a buffer of frames directed at the edges, built once per shape: -> (x, true starts, coarse starts, prs, zero frame)
    frame 0: m = -M, tau = 0;  1: m = +M, tau = 2W;  2: eps near +1/2;  3: eps near -1/2;  4: all-zero samples;  the rest
    random.  Leads alternate in parity, so coarse starts are odd and even.  uniform: equal chunks and one timing error, for
    the stride path."""
    key = (shape, nframes, uniform)
    if key in _cache:
        return _cache[key]
    nfft, G, nsyms, W, M = shape
    prm = Params(nfft, G, nsyms, W, M)
    rng = np.random.default_rng(900 + nfft + nframes)
    bins = std_bins(nfft)
    prs = prs_table(rng, nfft, bins)
    m = rng.integers(-max(M - 1, 0), max(M - 1, 0) + 1, nframes).astype(np.float64)  # |m + eps| <= M - 1/2
    eps = rng.uniform(-0.4, 0.4, nframes)
    delta = rng.integers(-W, W + 1, nframes)
    m[:4], eps[:4] = [-M, M, 0, min(1, M)], [0.3, -0.3, 0.499, -0.499]
    delta[:2] = [W, -W]
    if uniform:
        delta[:] = -W + 1 if W else 0
    lead = [2 * W + 2 + (0 if uniform else t % 2 + int(rng.integers(0, 3)) * 2) for t in range(nframes)]
    tail = [2 * W + 2] * nframes
    x, true, _ = transmit_frames(rng, prm, prs, bins, nframes, m + eps, lead=lead, tail=tail, snr_db=15.0)
    if nframes > 4:
        x[true[4] - G - lead[4]:true[4] - G + nsyms * (nfft + G) + tail[4]] = 0
    coarse = true + delta
    assert uniform or W == 0 or {int(c) % 2 for c in coarse} == {0, 1}
    _cache[key] = (x, true, coarse, prs)
    return _cache[key]


def run_sync(V, x, prm, prs, coarse, nframes, table=True, alias=False, nco_bits=12, with_info=True, nsamples=None,
             frame_stride=None, unspecified=(), device=None):
    """one call on guarded outputs; the whole buffers are compared with the model's image -> the model's outputs.
    unspecified: frames outside the header's domain - the model skips them, their words are not compared except that
    the start is an integer of c - W - backoff ... c + W - backoff (tau <= 2W), and the device's words are returned
    for them.  device: a dict that gets the device's words, without the guards: start, rot (n, 2), info (n, 8)"""
    nfft = prm.nfft
    tw, d_tw = tw_tables(V, nfft)
    nco, d_nco = nco_tables(V, nco_bits)
    d_iq = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_prs = torch.from_numpy(prs).cuda()
    so = torch.full((2 * GW + nframes,), SENT64, dtype=torch.int64, device="cuda")
    ro = dev_u32(np.full(2 * (2 * GW + nframes), SENT32, np.uint32))
    io = dev_u32(np.full(10 + 8 * nframes, SENT32, np.uint32))
    d_so = so[GW:GW + nframes]
    d_start = None
    if table:
        if alias:
            d_so.copy_(torch.from_numpy(np.asarray(coarse[:nframes], np.int64)))
            d_start = d_so
        else:
            d_start = torch.from_numpy(np.asarray(coarse[:nframes], np.int64)).cuda()
        assert d_start.data_ptr() % 8 == 0
    V.ofdm_sync_dev(d_iq, nfft, prm.nsyms, nframes, d_tw, prm.sym_stride, d_nco, nco_bits, d_prs, d_so, ro[2 * GW:], prm.W, prm.M,
                    cp_symbols=prm.cp_symbols, thr=prm.thr, backoff=prm.backoff, frame_stride=frame_stride,
                    first_start=0 if table else int(coarse[0]), d_start=d_start, d_info=io[5:] if with_info else None,
                    nsamples=nsamples)
    torch.cuda.synchronize()
    n = x.size if nsamples is None else nsamples
    bad = np.asarray(unspecified, np.int64)
    model_coarse = np.array(coarse[:nframes], np.int64)
    model_coarse[bad] = -1  # skipped by the model
    start, rot, info, turn = sync_model(x[:n], model_coarse, prm, prs, tw, nco, nco_bits)
    want_so = np.full(so.numel(), SENT64, np.int64)
    want_so[GW:GW + nframes] = start
    want_ro = np.full(ro.numel(), SENT32, np.uint32)
    want_ro[2 * GW:2 * GW + 2 * nframes] = rot.reshape(-1)
    want_io = np.full(io.numel(), SENT32, np.uint32)
    if with_info:
        want_io[5:5 + 8 * nframes] = info.reshape(-1)
    got_so, got_ro, got_io = so.cpu().numpy(), ro.cpu().numpy().view(np.uint32), io.cpu().numpy().view(np.uint32)
    if device is not None:
        device.update(start=got_so[GW:GW + nframes].copy(), rot=got_ro[2 * GW:2 * GW + 2 * nframes].reshape(-1, 2).copy(),
                      info=got_io[5:5 + 8 * nframes].reshape(-1, 8).copy())
    for t in bad:
        lo = int(coarse[t]) - prm.W - prm.backoff
        assert lo <= int(got_so[GW + t]) <= lo + 2 * prm.W, "the start of a frame outside the domain"
        start[t], rot[t] = got_so[GW + t], got_ro[2 * GW + 2 * t:2 * GW + 2 * t + 2]
        want_so[GW + t], want_ro[2 * GW + 2 * t:2 * GW + 2 * t + 2] = start[t], rot[t]
        if with_info:
            info[t] = got_io[5 + 8 * t:13 + 8 * t]
            got_io[5 + 8 * t:13 + 8 * t] = want_io[5 + 8 * t:13 + 8 * t]  # its floats may be NaN: not compared
    assert np.array_equal(got_so, want_so), "starts and their guards"
    assert np.array_equal(got_ro, want_ro), "rot and its guards"
    ints = np.zeros(io.numel(), bool)
    ints[5:5 + 8 * nframes] = np.tile(np.arange(8) < 2, nframes)
    assert np.array_equal(got_io[ints], want_io[ints]), "m^ and tau"
    # the six floats by value (-0 = +0), everything else bit for bit
    assert np.array_equal(got_io[~ints].view(np.float32), want_io[~ints].view(np.float32)), "info floats and the guards"
    return start, rot, info, turn


@pytest.mark.parametrize("shape", SHAPES)
def test_directed_frames_against_the_model(V, torch_cuda, shape):
    """1 and 3 frames and all 8, cp_symbols 1 and nsyms-1, thr 1 and 0.5, a backoff; the directed frames land where they
    were aimed"""
    nfft, G, nsyms, W, M = shape
    x, true, coarse, prs = directed(shape)
    prm = Params(nfft, G, nsyms, W, M, thr=0.5, backoff=3)
    start, rot, info, turn = run_sync(V, x, prm, prs, coarse, 8)
    mhat, tau = info[:, 0].view(np.int32), info[:, 1].view(np.int32)
    assert mhat[0] == -M and mhat[1] == M and tau[0] == 0 and tau[1] == 2 * W
    assert abs(abs(float(turn[2])) - 0.5) < 0.01 and abs(abs(float(turn[3])) - 0.5) < 0.01
    assert np.array_equal(start[[0, 1, 2, 3, 5, 6, 7]] + 3, true[[0, 1, 2, 3, 5, 6, 7]])
    # all-zero samples: ties everywhere
    assert mhat[4] == -M and tau[4] == 0 and turn[4] == 0 and not info[4, 2:].any() and start[4] == coarse[4] - W - 3
    assert rot[4].tolist() == [0, (M * ((1 << 32) // nfft)) % (1 << 32)]
    run_sync(V, x, Params(nfft, G, nsyms, W, M, cp_symbols=1, thr=1.0), prs, coarse, 3, nco_bits=20)
    run_sync(V, x, Params(nfft, G, nsyms, W, M, cp_symbols=nsyms - 1), prs, coarse, 1, with_info=False, nco_bits=1)
    run_sync(V, x, Params(nfft, G, nsyms, W, M, cp_symbols=min(2, nsyms - 1)), prs, coarse[::-1].copy(), 3, alias=True)


@pytest.mark.parametrize("shape", SHAPES[:2])
def test_seventy_frames(V, torch_cuda, shape):
    """more than one frame per CU slot and every lane of the table: the coarse table, then aliased by the output"""
    nfft, G, nsyms, W, M = shape
    x, true, coarse, prs = directed(shape, 70)
    prm = Params(nfft, G, nsyms, W, M)
    start = run_sync(V, x, prm, prs, coarse, 70)[0]
    keep = np.arange(70) != 4
    assert np.array_equal(start[keep], true[keep])
    run_sync(V, x, prm, prs, coarse, 70, alias=True)


@pytest.mark.parametrize("shape", [(64, 16, 4, 0, 3), (256, 63, 8, 15, 0), (512, 126, 5, 0, 0), (128, 3, 3, 1, 63)])
def test_no_uncertainty(V, torch_cuda, shape):
    """W = 0 (one candidate start), M = 0 (one shift), both; G - 2W = 1 with M = 63 at nfft 128 (the most shifts it allows)"""
    nfft, G, nsyms, W, M = shape
    x, true, coarse, prs = directed(shape)
    for cp in (1, nsyms - 1):
        run_sync(V, x, Params(nfft, G, nsyms, W, M, cp_symbols=cp), prs, coarse, 8)


@pytest.mark.parametrize("shape", [(128, 32, 4, 6, 5), (4096, 1008, 3, 50, 2), (8192, 600, 3, 64, 64)])
def test_other_lengths(V, torch_cuda, shape):
    """the lengths no mode uses: two accumulators' worth of points per thread at 128, 16 wavefronts at 8192 (more than 64 KB
    of LDS, the most shifts)"""
    nfft, G, nsyms, W, M = shape
    x, true, coarse, prs = directed(shape, 5)
    start = run_sync(V, x, Params(nfft, G, nsyms, W, M), prs, coarse, 5)[0]
    assert np.array_equal(start[:4], true[:4])


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]])
def test_stride_with_first_start(V, torch_cuda, shape):
    """no table: frame t starts at first_start + t*frame_stride; the buffer ends with the last frame's span"""
    nfft, G, nsyms, W, M = shape
    x, true, coarse, prs = directed(shape, 5, uniform=True)
    stride = int(true[1] - true[0])
    assert (np.diff(true) == stride).all()
    prm = Params(nfft, G, nsyms, W, M)
    for nframes in (1, 3, 5):
        n = int(coarse[nframes - 1]) - W + prm.span()
        start = run_sync(V, x, prm, prs, coarse, nframes, table=False, frame_stride=stride, nsamples=n)[0]
        assert (start != -1).all()


def test_skipped_frames(V, torch_cuda):
    """a coarse table whose spans leave the buffer at the front and at the back, by one sample and by far, next to
    frames that just fit: -1, {0, 0} and zeros for the skipped ones, the model's words for the others, the guards whole"""
    shape = SHAPES[1]
    nfft, G, nsyms, W, M = shape
    x, true, coarse, prs = directed(shape)
    prm = Params(nfft, G, nsyms, W, M)
    n = x.size - 7
    last = n - prm.span() + W  # the last coarse start whose span is inside
    table = np.array([W - 1, W, -1, last + 1, last, -(1 << 62), 1 << 62, n, int(coarse[1])], np.int64)
    for alias in (False, True):
        start = run_sync(V, x, prm, prs, table, table.size, alias=alias, nsamples=n)[0]
        assert ((start == -1) == np.array([1, 0, 1, 1, 0, 1, 1, 1, 0], bool)).all()


def test_argument_errors(V, torch_cuda):
    assert argument_error_cases(V, torch) > 40


def test_end_to_end_into_the_demodulator(V, torch_cuda):
    """noise-free mode-III frames with a start, an integer and a fractional offset per frame: vit_ofdm_sync_dev writes the
    two tables, vit_ofdm_demod_dev reads them as they are (nco_bits 12), every hard decision is the transmitted bit"""
    nfft, K, nsyms, fic_syms, cifs = MODE_III
    G, W, M, nframes, nco_bits = 63, 12, 6, 4, 12
    rng = np.random.default_rng(990)
    prm = Params(nfft, G, nsyms, W, M, cp_symbols=20, thr=0.5, backoff=G // 2)
    bins = freq_bins_model(nfft)[1]
    prs = prs_table(rng, nfft, bins)
    off = np.array([-5.5, 3.25, 0.49, 5.1])
    lead = [2 * W + 2 + int(v) for v in rng.integers(0, 50, nframes)]
    x, true, bits = transmit_frames(rng, prm, prs, bins, nframes, off, lead=lead)
    coarse = true + np.array([W, -W, 3, -4])
    d_iq = torch.from_numpy(x).cuda()
    d_tw, d_nco = tw_tables(V, nfft)[1], nco_tables(V, nco_bits)[1]
    d_start = torch.from_numpy(coarse).cuda()
    d_rot = dev_u32(np.zeros((nframes, 2), np.uint32))
    V.ofdm_sync_dev(d_iq, nfft, nsyms, nframes, d_tw, prm.sym_stride, d_nco, nco_bits, torch.from_numpy(prs).cuda(), d_start,
                    d_rot, W, M, cp_symbols=prm.cp_symbols, thr=prm.thr, backoff=prm.backoff, d_start=d_start)
    per = nsyms - 1 - fic_syms
    d_fic = torch.full((nframes, fic_syms * 2 * K), 128, dtype=torch.uint8, device="cuda")
    d_ring = torch.full((nframes * cifs, per * 2 * K), 128, dtype=torch.uint8, device="cuda")
    V.ofdm_demod_dev(d_iq, MODE_III, dev_bins(bins), 254.0, nframes, d_tw, prm.sym_stride, d_start=d_start, d_nco=d_nco,
                     nco_bits=nco_bits, d_rot=d_rot, d_fic=d_fic, d_ring=d_ring)
    torch.cuda.synchronize()
    assert np.array_equal(d_start.cpu().numpy(), true - prm.backoff)
    assert np.array_equal(d_fic.cpu().numpy() > 128, bits[:, :fic_syms].reshape(nframes, -1).astype(bool))
    assert np.array_equal(d_ring.cpu().numpy() > 128, bits[:, fic_syms:].reshape(nframes, -1).astype(bool))
