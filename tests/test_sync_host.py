"""CPU-only: "From the coarse start" (include/viterbi_amd.h) - the definition of vit_ofdm_sync_dev as a numpy float32 model
independent of the library (sync_model: one float32 ufunc per operation, the long sums in the header's grouping, the
transforms and the rotation those of tests/test_fft_host.py), the same estimator in float64 (sync_f64), and a transmitter
with a known QPSK phase reference symbol, silence in front of every frame, an optional echo and AWGN.  The model's
arctangent is pinned against float64 atan2, the model against the truth without noise and against sync_f64 with it, and
sync_f64 against the truth at 10 dB.  tests/test_gpu_sync.py uses sync_model as its exact reference."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from test_fft_host import F32, fft_model, nco_model, rotate_model, time_domain, twiddles_model

ATAN_C = [F32(float.fromhex(h)) for h in ("0x1.45f2b4p-3", "-0x1.b26414p-5", "0x1.0240f6p-5", "-0x1.591268p-6",
                                           "0x1.9f40a4p-7", "-0x1.5e8136p-8", "0x1.1c32c4p-10")]


class Params:
    """vit_sync_params and the strides of vit_iq_input it goes with"""

    def __init__(self, nfft, guard, nsyms, W, M, cp_symbols=None, thr=0.5, backoff=0):
        self.nfft, self.guard, self.nsyms, self.W, self.M = nfft, guard, nsyms, W, M
        self.cp_symbols = nsyms - 1 if cp_symbols is None else cp_symbols
        self.thr, self.backoff = thr, backoff
        self.sym_stride = nfft + guard

    def span(self):
        return (self.nsyms - 1) * self.sym_stride + self.nfft + 2 * self.W


# ---- the definition -------------------------------------------------------------------------------------------------

def nacc_of(nfft):
    return max(64, nfft // 8)


def long_sum(v, nacc):
    """v: (..., n) float32 -> (...): element e to accumulator e mod nacc in ascending e, then the tree of adjacent pairs"""
    assert v.dtype == F32
    n = v.shape[-1]
    rows = -(-n // nacc)
    p = np.zeros(v.shape[:-1] + (rows * nacc,), F32)
    p[..., :n] = v
    p = p.reshape(v.shape[:-1] + (rows, nacc))
    acc = np.zeros(v.shape[:-1] + (nacc,), F32)
    with np.errstate(all="ignore"):
        for r in range(rows):
            acc = acc + p[..., r, :]  # adding the padding's +0 changes no value
        while acc.shape[-1] > 1:
            acc = acc[..., 0::2] + acc[..., 1::2]
    assert acc.dtype == F32
    return acc[..., 0]


def mul_conj_model(ar, ai, br, bi):
    """a * conj(b): fl(fl(ar*br) + fl(ai*bi)), fl(fl(ai*br) - fl(ar*bi))"""
    assert ar.dtype == F32 and ai.dtype == F32 and br.dtype == F32 and bi.dtype == F32
    return ar * br + ai * bi, ai * br - ar * bi


def turn_model(re, im):
    """atan2(im, re) / 2 pi in [-1/2, 1/2], the header's graph on float32 arrays"""
    re, im = np.asarray(re, F32), np.asarray(im, F32)
    ax, ay = np.abs(re), np.abs(im)
    mx, mn = np.maximum(ax, ay), np.minimum(ax, ay)
    with np.errstate(all="ignore"):
        q = mn / np.where(mx > 0, mx, F32(1))
        s = q * q
        p = np.full_like(q, ATAN_C[6])
        for c in ATAN_C[5::-1]:
            p = p * s
            p = p + c
        r = p * q
        r = np.where(ay > ax, F32(0.25) - r, r)
        r = np.where(re < 0, F32(0.5) - r, r)
        r = np.where(im < 0, -r, r)
    r = np.where(mx > 0, r, F32(0))
    assert r.dtype == F32
    return r


def split(x):
    x = np.asarray(x, np.complex64)
    return np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)


def join(re, im):
    out = np.empty(re.shape, np.complex64)
    out.real, out.imag = re, im
    return out


def sync_model(x, coarse, prm, prs, tw, nco, nco_bits, detail=None):
    """x: the samples (complex64, 1-D); coarse: the frames' coarse starts -> (start int64 (n,), rot uint32 (n, 2), info
    uint32 (n, 8), turn float32 (n,)); a frame whose span is outside the buffer gets -1, {0, 0}, zeros.  detail: a list
    that gets, per frame that is not skipped, a dict of the intermediate values t, step_frac, metric and p"""
    x = np.asarray(x, np.complex64)
    nfft, S, G, W, M = prm.nfft, prm.sym_stride, prm.guard, prm.W, prm.M
    nacc, Gw = nacc_of(nfft), G - 2 * W
    scale = F32(2.0 ** 32 / nfft)
    pr, pi = split(prs)
    rr, ri = mul_conj_model(pr, pi, np.roll(pr, 1), np.roll(pi, 1))
    n = len(coarse)
    start, rot = np.full(n, -1, np.int64), np.zeros((n, 2), np.uint32)
    info, turns = np.zeros((n, 8), np.uint32), np.zeros(n, F32)
    with np.errstate(all="ignore"):
        for t, c in enumerate(int(v) for v in coarse):
            if c - W < 0 or c - W + prm.span() > x.size:
                continue
            # A
            idx = (c + np.arange(1, prm.cp_symbols + 1)[:, None] * S - G + W + np.arange(Gw)[None, :]).reshape(-1)
            ar, ai = split(x[idx])
            br, bi = split(x[idx + nfft])
            g_re = long_sum(ar * br + ai * bi, nacc)
            g_im = long_sum(ar * bi - ai * br, nacc)
            en = long_sum((ar * ar + ai * ai) + (br * br + bi * bi), nacc)
            turn = turn_model(g_re, g_im)
            step_frac = (-int(np.rint(turn * scale))) % (1 << 32)
            # B
            win = x[c - W:c - W + nfft].reshape(1, 1, nfft)
            yr, yi = split(fft_model(rotate_model(win, nco, nco_bits, [[0, step_frac]], S), tw)[0, 0])
            # C
            dr, di = mul_conj_model(yr, yi, np.roll(yr, 1), np.roll(yi, 1))
            sr = np.stack([np.roll(dr, -m) for m in range(-M, M + 1)])
            si = np.stack([np.roll(di, -m) for m in range(-M, M + 1)])
            cr, ci = mul_conj_model(sr, si, np.broadcast_to(rr, sr.shape), np.broadcast_to(ri, sr.shape))
            cr, ci = long_sum(np.ascontiguousarray(cr), nacc), long_sum(np.ascontiguousarray(ci), nacc)
            metric = cr * cr + ci * ci
            best = int(np.argmax(metric))  # the first maximum
            mhat = best - M
            # D
            zr, zi = mul_conj_model(np.roll(yr, -mhat), np.roll(yi, -mhat), pr, pi)
            hr, hi = split(fft_model(join(zr, -zi), tw))
            p = hr * hr + hi * hi
            psum = long_sum(p, nacc)
            pmax = p[:2 * W + 1].max()
            tau = int(np.argmax(p[:2 * W + 1] >= F32(prm.thr) * pmax))
            # E
            start[t] = c - W + tau - prm.backoff
            rot[t] = (0, (step_frac - mhat * ((1 << 32) // nfft)) % (1 << 32))
            info[t, :2] = np.array([mhat, tau], np.int32).view(np.uint32)
            info[t, 2:] = np.array([g_re, g_im, en, metric[best], pmax, psum], F32).view(np.uint32)
            turns[t] = turn
            if detail is not None:
                detail.append(dict(t=t, step_frac=step_frac, metric=metric, p=p))
    return start, rot, info, turns


def sync_f64(x, coarse, prm, prs):
    """the same estimator in float64 with np.angle and np.fft -> (start, mhat, turn)"""
    x = np.asarray(x, np.complex128)
    nfft, S, G, W, M = prm.nfft, prm.sym_stride, prm.guard, prm.W, prm.M
    P = np.asarray(prs, np.complex128)
    R = P * np.conj(np.roll(P, 1))
    out = []
    for c in (int(v) for v in coarse):
        idx = (c + np.arange(1, prm.cp_symbols + 1)[:, None] * S - G + W + np.arange(G - 2 * W)[None, :]).reshape(-1)
        turn = np.angle(np.sum(np.conj(x[idx]) * x[idx + nfft])) / (2 * np.pi)
        i = np.arange(nfft)
        Y = np.fft.fft(x[c - W:c - W + nfft] * np.exp(-2j * np.pi * turn * i / nfft))
        D = Y * np.conj(np.roll(Y, 1))
        metric = [abs(np.sum(np.roll(D, -m) * np.conj(R))) ** 2 for m in range(-M, M + 1)]
        mhat = int(np.argmax(metric)) - M
        h = np.conj(np.fft.fft(np.conj(np.roll(Y, -mhat) * np.conj(P))))
        p = np.abs(h[:2 * W + 1]) ** 2
        tau = int(np.argmax(p >= prm.thr * p.max()))
        out.append((c - W + tau - prm.backoff, mhat, turn))
    return (np.array([o[0] for o in out], np.int64), np.array([o[1] for o in out], np.int64),
            np.array([o[2] for o in out], np.float64))


def step_in_spacings(step, nfft):
    """the frequency offset a rotation step takes away, in carrier spacings"""
    s = np.asarray(step, np.int64)
    s = np.where(s >= 1 << 31, s - (1 << 32), s)
    return -s * nfft / 2.0 ** 32


# ---- the transmitter ------------------------------------------------------------------------------------------------

def prs_table(rng, nfft, bins):
    """a known QPSK phase reference symbol in FFT order, zero on unused bins"""
    P = np.zeros(nfft, np.complex64)
    P[np.asarray(bins, np.int64)] = np.exp(0.5j * np.pi * rng.integers(0, 4, len(bins))).astype(np.complex64)
    return P + np.complex64(0)  # -0 -> +0 after the cast


def std_bins(nfft):
    """the carriers of the standard's modes, DC left out: 3 nfft / 4 bins"""
    k = np.concatenate([np.arange(-3 * nfft // 8, 0), np.arange(1, 3 * nfft // 8 + 1)])
    return k % nfft


def transmit_frames(rng, prm, prs, bins, nframes, offsets, lead=None, tail=None, echo=None, snr_db=None, scale=None):
    """nframes frames of prm.nsyms symbols (the known reference symbol, then random DQPSK data on `bins`),
    frame t with a frequency offset of offsets[t] carrier spacings, lead[t] samples of silence in front and tail[t]
    behind; echo = (amplitude, delay) adds a second path inside every frame, AWGN at snr_db per carrier on everything ->
    (samples complex64, true starts int64: the first useful sample of every reference symbol, bits (nframes, nsyms-1, 2K))"""
    nfft, G, K = prm.nfft, prm.guard, len(bins)
    lead = [2 * prm.W + 2] * nframes if lead is None else lead
    tail = [2 * prm.W + 2] * nframes if tail is None else tail
    scale = 1.0 / nfft if scale is None else scale
    bits = rng.integers(0, 2, (nframes, prm.nsyms - 1, 2 * K))
    q = ((1 - 2 * bits[:, :, :K]) + 1j * (1 - 2 * bits[:, :, K:])) / np.sqrt(2.0)
    ref = np.broadcast_to(np.asarray(prs, np.complex128)[np.asarray(bins, np.int64)], (nframes, 1, K))
    z = np.zeros((nframes, prm.nsyms, nfft), np.complex128)
    z[:, :, np.asarray(bins, np.int64)] = np.concatenate([ref, q], axis=1).cumprod(axis=1)
    chunks, starts, pos = [], [], 0
    for t in range(nframes):
        f = time_domain(z[t:t + 1], G, offsets[t])[0]
        if echo is not None:
            amp, delay = echo[t] if isinstance(echo, list) else echo
            f = f + np.concatenate([np.zeros(delay), amp * f[:-delay]])
        chunks += [np.zeros(lead[t]), f, np.zeros(tail[t])]
        starts.append(pos + lead[t] + G)
        pos += lead[t] + f.size + tail[t]
    x = np.concatenate(chunks)
    if snr_db is not None:
        sigma = np.sqrt(nfft * 10.0 ** (-snr_db / 10.0) / 2.0)
        x = x + sigma * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))
    return (x * scale).astype(np.complex64), np.array(starts, np.int64), bits


def draw_offsets(rng, n, M):
    """integer offsets m and fractional offsets eps per frame with |m + eps| <= M - 1/2"""
    m = rng.integers(-M + 1, M, n) if M > 0 else np.zeros(n, np.int64)
    eps = rng.uniform(-0.5, 0.5, n)
    if M == 0:
        eps = rng.uniform(-0.45, 0.45, n)
    else:
        assert (np.abs(m + eps) <= M - 0.5).all()
    return m, eps


# ---- the arctangent ---------------------------------------------------------------------------------------------------

def test_turn_against_float64_atan2():
    """dense angles, magnitudes 2^-40 ... 2^40: within 2^-18 turn (0.13 degrees of drift over a mode-I frame); the axes,
    the diagonals and 0 exactly"""
    rng = np.random.default_rng(11)
    a = np.concatenate([np.linspace(-np.pi, np.pi, 400001), rng.uniform(-np.pi, np.pi, 400000)])
    mag = 2.0 ** np.concatenate([rng.uniform(-40, 40, a.size - 162), np.repeat(np.arange(-40, 41), 2)])
    re, im = (mag * np.cos(a)).astype(F32), (mag * np.sin(a)).astype(F32)
    t = turn_model(re, im).astype(np.float64)
    ref = np.arctan2(im.astype(np.float64), re.astype(np.float64)) / (2 * np.pi)
    d = np.abs(t - ref)
    d = np.minimum(d, 1.0 - d)
    print("arctangent: at most %.4f x 2^-18 turn" % (d.max() / 2.0 ** -18))
    assert d.max() <= 2.0 ** -18
    assert np.abs(t).max() <= 0.5
    # components of very different magnitude
    re = np.array([2.0 ** 40, 2.0 ** -40, -2.0 ** 40, 2.0 ** -40, -2.0 ** -40], F32)
    im = np.array([2.0 ** -40, 2.0 ** 40, 2.0 ** -40, -2.0 ** 40, -2.0 ** 40], F32)
    ref = np.arctan2(im.astype(np.float64), re.astype(np.float64)) / (2 * np.pi)
    assert np.abs(turn_model(re, im) - ref).max() <= 2.0 ** -18
    exact = turn_model(np.array([0, 1, 0, -1, 0, 3, -3, -3, 3], F32), np.array([0, 0, 1, 0, -1, 3, 3, -3, -3], F32))
    assert np.abs(exact - np.array([0, 0, 0.25, 0.5, -0.25, 0.125, 0.375, -0.375, -0.125])).max() <= 2.0 ** -23


def test_long_sum_grouping():
    """the grouping is the header's: round robin to the accumulators, then adjacent pairs"""
    v = np.arange(1, 201, dtype=np.float64)
    assert long_sum(v.astype(F32), 64) == v.sum()
    # a sum whose value depends on the grouping: 2^24 absorbs single ones but not their pairwise sums
    v = np.ones(128, F32)
    v[0] = 2.0 ** 24
    assert long_sum(v, 64) == F32(2.0 ** 24 + 126)  # accumulator 0 loses its one, the other 63 hold 2 each and meet first
    seq = F32(0)
    for e in v:
        seq = seq + e
    assert seq == F32(2.0 ** 24)  # a sequential sum loses every one


# ---- the model against the truth and against float64 ---------------------------------------------------------------

def run_models(rng, prm, nframes, snr_db=None, echo=False, nco_bits=16):
    bins = std_bins(prm.nfft)
    prs = prs_table(rng, prm.nfft, bins)
    m, eps = draw_offsets(rng, nframes, prm.M)
    echoes = None
    if echo:
        echoes = [(0.5 * np.exp(2j * np.pi * rng.random()), int(rng.integers(1, (prm.guard + 3) // 4))) for _ in range(nframes)]
    x, true, _ = transmit_frames(rng, prm, prs, bins, nframes, m + eps, echo=echoes, snr_db=snr_db)
    coarse = true + rng.integers(-prm.W, prm.W + 1, nframes)
    tw, nco = twiddles_model(prm.nfft), nco_model(nco_bits)
    return x, true, coarse, prs, m + eps, sync_model(x, coarse, prm, prs, tw, nco, nco_bits), sync_f64(x, coarse, prm, prs)


@pytest.mark.parametrize("nfft,guard,nsyms,W,M,nframes", [(256, 63, 8, 15, 8, 24), (64, 16, 4, 4, 3, 12), (2048, 504, 6, 100, 16, 3)])
def test_noise_free_single_path(nfft, guard, nsyms, W, M, nframes):
    """every start exact, the frequency within 2^-16 spacing (four times the arctangent's bound: the rest is the rounding
    accumulated in gamma)"""
    rng = np.random.default_rng(20 + nfft)
    prm = Params(nfft, guard, nsyms, W, M)
    x, true, coarse, prs, off, (start, rot, info, turn), _ = run_models(rng, prm, nframes)
    mhat = info[:, 0].view(np.int32)
    err = np.abs(mhat + turn.astype(np.float64) - off)
    print("nfft %d: frequency error at most %.3f x 2^-16 spacing" % (nfft, err.max() / 2.0 ** -16))
    assert np.array_equal(start, true)
    assert err.max() <= 2.0 ** -16
    assert np.abs(step_in_spacings(rot[:, 1], nfft) - off).max() <= 2.0 ** -16 + nfft / 2.0 ** 33
    assert (rot[:, 0] == 0).all()


def test_noise_and_echo_against_float64():
    """10 dB, an echo at -6 dB delayed by under a quarter of the guard, thr 0.5: the model agrees with float64 on every
    start and every integer offset and within 2^-16 spacing in frequency; float64 finds the first path in every frame
    with a frequency error under 0.02 spacing (9 degrees between consecutive symbols against DQPSK's 45)"""
    rng = np.random.default_rng(31)
    prm = Params(256, 63, 8, 15, 8, thr=0.5)
    x, true, coarse, prs, off, (start, rot, info, turn), (start64, mhat64, turn64) = run_models(rng, prm, 40, 10.0, True)
    mhat = info[:, 0].view(np.int32)
    d = np.abs((mhat + turn.astype(np.float64)) - (mhat64 + turn64))
    err64 = np.abs(mhat64 + turn64 - off)
    print("wrong starts %d of 40, frequency error at most %.4f spacing, model against float64 %.3f x 2^-16"
          % (int((start64 != true).sum()), err64.max(), d.max() / 2.0 ** -16))
    assert np.array_equal(start, start64) and np.array_equal(mhat, mhat64)
    assert d.max() <= 2.0 ** -16
    assert np.array_equal(start64, true)
    assert err64.max() < 0.02


def test_skip_rule_and_backoff_in_the_model():
    """a span outside the buffer gives -1, {0, 0}, zeros; backoff moves the start only"""
    rng = np.random.default_rng(41)
    prm = Params(64, 16, 4, 4, 3, backoff=5)
    bins = std_bins(64)
    prs = prs_table(rng, 64, bins)
    x, true, _ = transmit_frames(rng, prm, prs, bins, 1, [0.0], lead=[4], tail=[4])
    tw, nco = twiddles_model(64), nco_model(12)
    assert true[0] - 4 == 16 and x.size == true[0] - 4 - 16 + 16 + prm.span()
    start, rot, info, _ = sync_model(x, [true[0] - 1, true[0], true[0] + 1, -3], prm, prs, tw, nco, 12)
    assert start.tolist() == [true[0] - 5, true[0] - 5, -1, -1]
    assert not rot[2:].any() and not info[2:].any() and info[0].any()


# ---- the library without a GPU --------------------------------------------------------------------------------------

def test_sync_export(V):
    out = subprocess.check_output(["nm", "-D", "--defined-only", V.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert "vit_ofdm_sync_dev" in exported and "vit_ofdm_sync_dev" in V.EXPORTS
    assert C.sizeof(V.SyncParams) == 40 and V.SyncParams.thr.offset == 20 and V.SyncParams.first_start.offset == 32
    assert callable(V.ofdm_sync_dev)


def argument_error_cases(V, torch):
    """every rule of vit_ofdm_sync_dev that is VIT_ERR_ARG, on a device: -> the number of cases checked"""
    L = V.lib()
    nfft, G, nsyms, W = 256, 63, 8, 15
    S = nfft + G
    fs = nsyms * S + 100
    d_iq = torch.zeros(2 * (3 * fs) + 8, dtype=torch.float32, device="cuda")
    d_tw = torch.from_numpy(V.fft_twiddles(nfft)).cuda()
    d_nco = torch.from_numpy(V.nco_table(10)).cuda()
    d_prs = torch.zeros(2 * nfft + 2, dtype=torch.float32, device="cuda")
    d_start = torch.full((2,), 100, dtype=torch.int64, device="cuda")
    d_so = torch.full((4,), 7, dtype=torch.int64, device="cuda")
    d_ro = torch.full((8,), 7, dtype=torch.int32, device="cuda")
    d_info = torch.full((17,), 7, dtype=torch.int32, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    span = (nsyms - 1) * S + nfft + 2 * W

    def call(inp=None, par=None, prs=P(d_prs), nframes=2, so=P(d_so), ro=P(d_ro), info=P(d_info), null_in=False, null_p=False):
        a = V.iq_input(d_iq, d_tw, S, fs, d_nco=d_nco, nco_bits=10, nsamples=3 * fs)
        for k, v in (inp or {}).items():
            setattr(a, k, v.value if isinstance(v, C.c_void_p) else v)
        p = dict(nfft=nfft, nsyms=nsyms, cp_symbols=nsyms - 1, W=W, M=8, thr=0.5, backoff=0, first_start=W)
        p.update(par or {})
        sp = V.SyncParams(p["nfft"], p["nsyms"], p["cp_symbols"], p["W"], p["M"], p["thr"], p["backoff"], p["first_start"])
        return L.vit_ofdm_sync_dev(None if null_in else C.byref(a), None if null_p else C.byref(sp), prs, nframes, so, ro, info, s)

    bad = [dict(null_in=True), dict(null_p=True), dict(prs=None), dict(so=None), dict(ro=None), dict(nframes=-1),
           dict(inp=dict(d_iq=None)), dict(inp=dict(d_tw=None)), dict(inp=dict(d_nco=None)),
           dict(inp=dict(d_iq=P(d_iq, 4))), dict(inp=dict(d_tw=P(d_tw, 4))), dict(inp=dict(d_nco=P(d_nco, 4))),
           dict(inp=dict(d_start=P(d_start, 4))), dict(prs=P(d_prs, 4)), dict(so=P(d_so, 4)), dict(ro=P(d_ro, 4)),
           dict(info=P(d_info, 2)), dict(inp=dict(nco_bits=0)), dict(inp=dict(nco_bits=21)), dict(inp=dict(d_rot=P(d_ro))),
           dict(par=dict(nfft=32)), dict(par=dict(nfft=250)), dict(par=dict(nfft=16384)), dict(par=dict(nsyms=1)),
           dict(par=dict(nsyms=0)), dict(par=dict(cp_symbols=0)), dict(par=dict(cp_symbols=nsyms)),
           dict(par=dict(W=32)), dict(par=dict(W=31, first_start=31), inp=dict(sym_stride=nfft + 62)),
           dict(inp=dict(sym_stride=nfft)), dict(inp=dict(sym_stride=nfft - 1)), dict(inp=dict(sym_stride=nfft + (1 << 31))),
           dict(par=dict(nfft=64, W=32, M=3), inp=dict(sym_stride=64 + 100)), dict(par=dict(M=65)),
           dict(par=dict(nfft=64, M=32, W=4), inp=dict(sym_stride=80)), dict(par=dict(thr=0.0)), dict(par=dict(thr=-0.5)),
           dict(par=dict(thr=1.5)), dict(par=dict(thr=float("nan"))), dict(par=dict(nsyms=1 << 31), inp=dict(sym_stride=1 << 40)),
           dict(par=dict(first_start=W - 1)), dict(par=dict(first_start=-1)), dict(nframes=3, par=dict(first_start=fs)),
           dict(inp=dict(nsamples=fs + span - 1)), dict(inp=dict(frame_stride=1 << 63)), dict(inp=dict(nsamples=0)),
           dict(par=dict(first_start=1 << 62))]
    for kw in bad:
        assert call(**kw) == 1, kw
        assert "bad arguments" in V.last_error(), kw
    assert call(nframes=0) == 0
    torch.cuda.synchronize()
    assert bool((d_so == 7).all()) and bool((d_ro == 7).all()) and bool((d_info == 7).all())
    # what is allowed: the buffer may end with the last frame's span, no d_info, W = 0, M = 0, thr = 1, a start table
    assert call() == 0 and call(inp=dict(nsamples=fs + span)) == 0 and call(info=None) == 0
    assert call(par=dict(W=0, first_start=0)) == 0 and call(par=dict(M=0)) == 0 and call(par=dict(thr=1.0)) == 0
    assert call(inp=dict(d_start=P(d_start), frame_stride=1 << 63), par=dict(first_start=-5)) == 0
    assert call(inp=dict(d_start=P(d_start), nsamples=5)) == 0  # both frames are skipped on the device
    torch.cuda.synchronize()
    assert d_so[:2].tolist() == [-1, -1] and d_ro[:4].tolist() == [0, 0, 0, 0] and not bool(d_info[:16].any())
    assert d_so[2:].tolist() == [7, 7] and d_ro[4:].tolist() == [7] * 4 and int(d_info[16]) == 7
    with pytest.raises(ValueError):
        V.ofdm_sync_dev(d_iq, nfft, nsyms, 1, d_tw, S, d_nco, 10, d_prs, d_so, d_ro, W, 8)  # neither frame_stride nor d_start
    with pytest.raises(ValueError):
        V.ofdm_sync_dev(d_iq, nfft, nsyms, 1, d_tw, S, None, 10, d_prs, d_so, d_ro, W, 8, frame_stride=fs)
    with pytest.raises(ValueError):
        V.ofdm_sync_dev(d_iq, nfft, nsyms, 1, d_tw, S, d_nco, 10, d_prs, d_so.to(torch.int32), d_ro, W, 8, frame_stride=fs)
    with pytest.raises(ValueError):
        V.ofdm_sync_dev(d_iq, nfft, nsyms, 1, d_tw, S, d_nco, 10, d_prs[:100], d_so, d_ro, W, 8, frame_stride=fs)
    return len(bad)


def test_sync_call_fails_loudly(V):
    """without a device: VIT_ERR_NO_DEVICE first, whatever the arguments, and an error text naming gfx950 - nothing is
    launched; with one, every argument rule is VIT_ERR_ARG"""
    import torch
    if torch.cuda.is_available():
        assert argument_error_cases(V, torch) > 40
        return
    inp = V.IqInput()
    inp.sym_stride, inp.frame_stride = 2552, 196608
    par = V.SyncParams(2048, 76, 75, 64, 16, 0.5, 0, 0)
    for args in ((C.byref(inp), C.byref(par)), (None, None), (C.byref(inp), None)):
        assert V.lib().vit_ofdm_sync_dev(args[0], args[1], None, 1, None, None, None, None) == 2
        assert "gfx950" in V.last_error()
    assert V.lib().vit_ofdm_sync_dev(None, None, None, -1, None, None, None, None) == 2
