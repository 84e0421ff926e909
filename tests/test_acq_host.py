"""CPU-only: "From the stream: first acquisition" (include/viterbi_amd.h) - the definition of vit_ofdm_acquire_dev as a numpy
float32 model independent of the library (acquire_model: one float32 ufunc per operation, a block's power in the tree of
adjacent pairs, a window's sum serial in ascending order, the last minimum per period) and the same estimator in float64
(acquire_f64).  The streams are those of tests/test_sync_host.py's transmitter with `lead` as the null symbol and equal
periods.  The model is pinned against the truth without noise (the edge's block, exactly) and against acquire_f64 with
it, and its table is handed to sync_model.  tests/test_gpu_acq.py uses acquire_model as its exact reference."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from test_fft_host import F32, nco_model, twiddles_model
from test_iqfmt_host import convert_model
from test_sync_host import Params, prs_table, std_bins, sync_model, transmit_frames

NONE = 0xFFFFFFFF


class Acq:
    """vit_acq_params"""

    def __init__(self, B, Ln, Lr, Pb, thr=None, first=0, offset=0):
        self.B, self.Ln, self.Lr, self.Pb, self.first, self.offset = B, Ln, Lr, Pb, first, offset
        self.thr = 0.5 * Ln / Lr if thr is None else thr  # q is Ln/Lr inside the signal


# ---- the definition -------------------------------------------------------------------------------------------------

def block_power_model(x, B):
    """x: complex64 (nblk*B,) -> float32 (nblk,): e = fl(fl(re*re) + fl(im*im)), then the tree of adjacent pairs"""
    x = np.asarray(x, np.complex64)
    re, im = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
    assert re.dtype == F32 and im.dtype == F32
    with np.errstate(all="ignore"):
        v = (re * re + im * im).reshape(-1, B)
        while v.shape[1] > 1:
            v = v[:, 0::2] + v[:, 1::2]
    assert v.dtype == F32
    return v[:, 0]


def window_sums_model(p, L, lo, n):
    """float32 (n,): element c is the sum of p[lo + c + i], i = 0 ... L-1, ascending, in one accumulator from +0"""
    assert p.dtype == F32
    acc = np.zeros(n, F32)
    with np.errstate(all="ignore"):
        for i in range(L):
            acc = acc + p[lo + i:lo + i + n]
    assert acc.dtype == F32
    return acc


def acquire_model(x, a, nperiods, nsamples=None):
    """x: the samples (complex64, 1-D); a: Acq -> (start int64 (n,), info uint32 (n, 4), p float32 (nblk,))"""
    x = np.asarray(x, np.complex64)
    n = x.size if nsamples is None else nsamples
    nblk = (n - a.first) // a.B
    p = block_power_model(x[a.first:a.first + nblk * a.B], a.B)
    ncand = max(nblk - a.Lr - a.Ln + 1, 0)  # candidates j = Ln + c
    N, R = window_sums_model(p, a.Ln, 0, ncand), window_sums_model(p, a.Lr, a.Ln, ncand)
    with np.errstate(all="ignore"):
        q = np.where(R > 0, N / np.where(R > 0, R, F32(1)), F32(np.inf)).astype(F32)
    start = np.full(nperiods, -1, np.int64)
    info = np.zeros((nperiods, 4), np.uint32)
    info[:, 0], info[:, 1] = NONE, np.array([np.inf], F32).view(np.uint32)[0]
    for k in range(min(nperiods, -(-ncand // a.Pb))):
        qk = q[k * a.Pb:(k + 1) * a.Pb]
        i = qk.size - 1 - int(np.argmin(qk[::-1]))  # the last minimum
        c = k * a.Pb + i
        info[k, 0] = i
        info[k, 1:] = np.array([q[c], N[c], R[c]], F32).view(np.uint32)
        if q[c] <= F32(a.thr):
            start[k] = a.first + (a.Ln + c) * a.B + a.offset
    return start, info, p


def acquire_f64(x, a, nperiods):
    """the same estimator in float64 -> start int64 (n,)"""
    x = np.asarray(x, np.complex128)
    nblk = (x.size - a.first) // a.B
    p = (np.abs(x[a.first:a.first + nblk * a.B]) ** 2).reshape(nblk, a.B).sum(axis=1)
    cs = np.concatenate([[0.0], np.cumsum(p)])
    j = np.arange(a.Ln, nblk - a.Lr + 1)
    N, R = cs[j] - cs[j - a.Ln], cs[j + a.Lr] - cs[j]
    with np.errstate(all="ignore"):
        q = np.where(R > 0, N / np.where(R > 0, R, 1.0), np.inf)
    start = np.full(nperiods, -1, np.int64)
    for k in range(min(nperiods, -(-j.size // a.Pb))):
        qk = q[k * a.Pb:(k + 1) * a.Pb]
        i = qk.size - 1 - int(np.argmin(qk[::-1]))
        if qk[i] <= a.thr:
            start[k] = a.first + (a.Ln + k * a.Pb + i) * a.B + a.offset
    return start


# ---- the streams ----------------------------------------------------------------------------------------------------

def null_stream(rng, prm, nperiods, null, lead0, snr_db=None, tail=64):
    """nperiods frames of prm with `null` samples of silence in front of each - lead0 in front of the first - and `tail`
    behind the last: equal periods of null + nsyms*sym_stride samples -> (x, edges: the first sample of every frame's
    first guard, true starts, prs)"""
    bins = std_bins(prm.nfft)
    prs = prs_table(rng, prm.nfft, bins)
    lead = [lead0] + [null] * (nperiods - 1)
    x, true, _ = transmit_frames(rng, prm, prs, bins, nperiods, [0.0] * nperiods, lead=lead, tail=[0] * (nperiods - 1) + [tail],
                                 snr_db=snr_db)
    return x, true - prm.guard, true, prs


# the noise test's stream, which tests/test_gpu_acq.py runs through the device chain: mode-III-like frames of 2552 samples
# behind nulls of 336, periods of 2888 = 361 blocks of 8; every edge in the middle of its block, so offset = guard + B/2
# makes a noise-free start exact
NOISE_SHAPE = (256, 63, 8)  # nfft, guard, nsyms
NOISE_ACQ = dict(B=8, Ln=32, Lr=16, Pb=361)
NOISE_PERIODS, NOISE_SNR_DB, NOISE_SEED, NOISE_W = 6, 10.0, 5, 16
_noise = {}


def noise_case():
    """-> (x, true starts, prs, prm with W = NOISE_W, Acq), built once"""
    if not _noise:
        nfft, G, nsyms = NOISE_SHAPE
        prm = Params(nfft, G, nsyms, NOISE_W, 4)
        rng = np.random.default_rng(NOISE_SEED)
        x, edges, true, prs = null_stream(rng, prm, NOISE_PERIODS, 336, 336 + 4, snr_db=NOISE_SNR_DB)
        assert (np.diff(edges) == 2888).all() and (edges % 8 == 4).all()
        _noise["case"] = (x, true, prs, prm, Acq(offset=G + 4, **NOISE_ACQ))
    return _noise["case"]


# ---- the model ------------------------------------------------------------------------------------------------------

def test_sum_groupings():
    """a block's sum is the tree of adjacent pairs, a window's sum is serial: each on values where the other grouping
    gives another result (2^24 absorbs single ones but not their pairwise sums)"""
    x = np.ones(16, np.complex64)
    x[0] = 4096.0  # e = 2^24
    assert block_power_model(np.arange(1, 17).astype(np.complex64), 16)[0] == F32(sum(i * i for i in range(1, 17)))
    assert block_power_model(x, 16)[0] == F32(2.0 ** 24 + 14)  # e[1] is lost against e[0], the other 14 meet in pairs first
    assert block_power_model(x, 8).tolist() == [2.0 ** 24 + 6, 8.0]
    # the window: 2^24, then ones - serially every one is lost; pairs first would keep them
    p = np.array([2.0 ** 24] + [1.0] * 8, F32)
    assert window_sums_model(p, 9, 0, 1)[0] == F32(2.0 ** 24)
    assert window_sums_model(p[::-1].copy(), 9, 0, 1)[0] == F32(2.0 ** 24 + 8)  # ascending order: the ones meet first
    # both in the estimator: N of candidate 9 is the serial sum, R the single block behind it
    s = np.zeros(10 * 2, np.complex64)
    s[0], s[2:18:2], s[18] = 4096.0, 1.0, 4096.0
    start, info, pw = acquire_model(s, Acq(2, 9, 1, 5, thr=4.0), 1)
    assert pw[1:9].tolist() == [1.0] * 8 and pw[9] == 2.0 ** 24
    assert pw[0] == 2.0 ** 24 and info[0, 0] == 0 and info[0, 1:].view(F32).tolist() == [1.0, 2.0 ** 24, 2.0 ** 24] and start[0] == 18


@pytest.mark.parametrize("B,lead0", [(8, 128), (8, 131), (32, 128), (32, 128 + 17), (32, 128 + 31)])
def test_noise_free_edges(B, lead0):
    """every period accepted and the edge inside the block the start names, exactly: 0 <= edge - (start - offset) < B;
    an edge at a block boundary (lead0 a multiple of B) and edges in mid-block"""
    nfft, G, nsyms = 64, 16, 4
    prm = Params(nfft, G, nsyms, 4, 3)
    frame = nsyms * (nfft + G)
    null = 128
    assert (null + frame) % B == 0 and null >= 2 * B
    a = Acq(B, null // B - 1, 2, (null + frame) // B, offset=-5)
    x, edges, _, _ = null_stream(np.random.default_rng(50 + lead0), prm, 5, null, lead0)
    start, info, _ = acquire_model(x, a, 5)
    d = edges - (start - a.offset)
    assert (start != -1).all() and (d >= 0).all() and (d < B).all(), d
    assert (d == lead0 % B).all() and not info[:, 1].any() and not info[:, 2].any()  # q = N = 0: the tie, its last member
    assert np.array_equal(start, acquire_f64(x, a, 5))
    # the same stream searched from an odd sample on: the blocks move, the edges stay
    b = Acq(B, a.Ln, 2, a.Pb, first=3, offset=-5)
    s3 = acquire_model(x, b, 5)[0]
    d = edges - (s3 - b.offset)
    assert (s3 != -1).all() and (d == (lead0 - 3) % B).all()


def test_noise_against_float64_and_into_the_synchroniser():
    """10 dB: acquire_f64 alone accepts every period and puts every start within B of the truth - on this stream it hits
    every edge's block, so with the edges in mid-block and offset = guard + B/2 the starts are exact: the bound |error| <= B
    is met with a block to spare on either side.  The float32 model is held to the same bound, and sync_model, fed its
    table with W = 16 >= B (no bias: the edges sit in the middle of their blocks), returns every true start."""
    x, true, prs, prm, a = noise_case()
    s64 = acquire_f64(x, a, NOISE_PERIODS)
    print("float64 errors", (s64 - true).tolist())
    assert (s64 != -1).all() and (np.abs(s64 - true) <= a.B).all()
    assert np.array_equal(s64, true), "the stream was chosen so that float64 hits every block"
    start, info, _ = acquire_model(x, a, NOISE_PERIODS)
    q = info[:, 1].view(F32)
    print("float32 errors", (start - true).tolist(), "q", q.tolist(), "thr", a.thr)
    assert (start != -1).all() and (np.abs(start - true) <= a.B).all()
    assert np.array_equal(start, s64)  # what the device chain of tests/test_gpu_acq.py builds on
    assert prm.W >= a.B and 2 * prm.W < prm.guard
    fine = sync_model(x, start, prm, prs, twiddles_model(prm.nfft), nco_model(12), 12)[0]
    assert np.array_equal(fine, true)
    # inside the signal q is about Ln/Lr, twice the threshold: the next period's table entry does not depend on luck
    assert q.max() < 0.5 * a.thr


def test_last_minimum_of_two_equal_nulls():
    """two nulls of exact zeros inside one period tie at q = 0: the later one's edge wins; with the second null removed
    the first one's edge does"""
    rng = np.random.default_rng(61)
    B, Ln, Lr, Pb = 8, 2, 2, 40
    x = (rng.standard_normal(Pb * B) + 1j * rng.standard_normal(Pb * B)).astype(np.complex64)
    x[5 * B:9 * B] = 0
    x[20 * B + 3:26 * B + 5] = 0
    a = Acq(B, Ln, Lr, Pb)
    start, info, _ = acquire_model(x, a, 1)
    assert start[0] == 26 * B and info[0, 0] == 26 - Ln and info[0, 1] == 0
    x[20 * B:27 * B] = 1.0
    assert acquire_model(x, a, 1)[0][0] == 9 * B


def test_edge_cases_of_the_model():
    """the all-zero stream (every q +Inf, j* the period's last candidate, start -1), a period without candidates, a
    partial last period, nblk = 0"""
    inf = np.array([np.inf], F32).view(np.uint32)[0]
    B, Ln, Lr, Pb = 8, 3, 2, 10
    a = Acq(B, Ln, Lr, Pb)
    z = np.zeros(25 * B + 5, np.complex64)  # 25 blocks: candidates 3 ... 23, 21 of them: periods of 10, 10 and 1
    start, info, p = acquire_model(z, a, 4)
    assert start.tolist() == [-1] * 4 and p.size == 25 and not p.any()
    assert info.tolist() == [[9, inf, 0, 0], [9, inf, 0, 0], [0, inf, 0, 0], [NONE, inf, 0, 0]]
    # a partial period holds a real edge; the period behind it has no candidate
    rng = np.random.default_rng(62)
    x = (rng.standard_normal(z.size) + 1j * rng.standard_normal(z.size)).astype(np.complex64)
    x[19 * B:23 * B + 2] = 0  # the edge in block 23, the last period's only candidate
    start, info, _ = acquire_model(x, a, 4)
    assert start[2] == 23 * B and info[2].tolist() == [0, 0, 0, info[2, 3]] and info[2, 3:].view(F32)[0] > 0
    assert start[3] == -1 and info[3].tolist() == [NONE, inf, 0, 0]
    # nothing to search: fewer samples than one block, first = nsamples, too few blocks for one candidate
    for xs, first in ((z[:7], 0), (z[:40], 40), (z[:4 * B], 0)):
        start, info, p = acquire_model(xs, Acq(B, Ln, Lr, Pb, first=first), 2)
        assert start.tolist() == [-1, -1] and info.tolist() == [[NONE, inf, 0, 0]] * 2 and p.size == (xs.size - first) // B
    # nsamples in mid-block: what lies behind it is not read
    y = x.copy()
    y[21 * B + 3:] = np.nan
    s1, i1, p1 = acquire_model(y, a, 3, nsamples=21 * B + 3)
    s2, i2, p2 = acquire_model(x[:21 * B], a, 3)
    assert np.array_equal(s1, s2) and np.array_equal(i1, i2) and np.array_equal(p1, p2) and p1.size == 21


def test_integer_formats_in_the_model():
    """an integer stream is searched as the floats of "Integer sample formats": a CU8 null is never exact zeros, and the
    edge is found all the same"""
    from test_iqfmt_host import IQ_CU8, quantise
    rng = np.random.default_rng(63)
    x = rng.standard_normal(60 * 8) + 1j * rng.standard_normal(60 * 8)
    x[10 * 8:30 * 8 + 4] *= 0.01
    raw, scale = quantise(x, IQ_CU8)
    start, info, _ = acquire_model(convert_model(raw, IQ_CU8, scale), Acq(8, 8, 4, 60), 1)
    assert start[0] == 30 * 8 and 0 < info[0, 1:2].view(F32)[0] < 0.05


# ---- the library without a GPU --------------------------------------------------------------------------------------

def test_acquire_export(V):
    out = subprocess.check_output(["nm", "-D", "--defined-only", V.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert "vit_ofdm_acquire_dev" in exported and "vit_ofdm_acquire_dev" in V.EXPORTS
    P = V.AcqParams
    assert C.sizeof(P) == 40 and [getattr(P, f).offset for f, _ in P._fields_] == [0, 4, 8, 12, 16, 20, 24, 32]
    assert callable(V.ofdm_acquire_dev)


def argument_error_cases(V, torch):
    """every rule of vit_ofdm_acquire_dev that is VIT_ERR_ARG, on a device: -> the number of cases checked"""
    L = V.lib()
    n = 4096
    d_iq = torch.zeros(2 * n + 8, dtype=torch.float32, device="cuda")
    d_so = torch.full((4,), 7, dtype=torch.int64, device="cuda")
    d_info = torch.full((13,), 7, dtype=torch.int32, device="cuda")
    d_pw = torch.full((n // 8 + 2,), 7.0, dtype=torch.float32, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731

    def call(iq=P(d_iq), nsamples=n, fmt=None, par=None, nperiods=2, so=P(d_so), info=P(d_info), pw=P(d_pw), null_p=False):
        p = dict(B=8, null_blocks=4, ref_blocks=2, period_blocks=100, thr=0.5, reserved=0, first=0, offset=0)
        p.update(par or {})
        ap = V.AcqParams(*[p[f] for f, _ in V.AcqParams._fields_])
        f = None if fmt is None else C.byref(V.IqFormat(*fmt))
        return L.vit_ofdm_acquire_dev(iq, nsamples, f, None if null_p else C.byref(ap), nperiods, so, info, pw, s)

    inf, nan = float("inf"), float("nan")
    bad = [dict(iq=None), dict(null_p=True), dict(so=None), dict(nperiods=-1),
           dict(iq=P(d_iq, 4)), dict(iq=P(d_iq, 2), fmt=(V.IQ_CU8, 1.0)), dict(iq=P(d_iq, 2), fmt=(V.IQ_CS16, 1.0)),
           dict(so=P(d_so, 4)), dict(info=P(d_info, 2)), dict(pw=P(d_pw, 2)),
           dict(par=dict(B=4)), dict(par=dict(B=0)), dict(par=dict(B=24)), dict(par=dict(B=1024)),
           dict(par=dict(null_blocks=0)), dict(par=dict(null_blocks=4097)), dict(par=dict(ref_blocks=0)),
           dict(par=dict(ref_blocks=4097)), dict(par=dict(period_blocks=0)), dict(par=dict(thr=0.0)), dict(par=dict(thr=-1.0)),
           dict(par=dict(thr=inf)), dict(par=dict(thr=nan)), dict(par=dict(reserved=1)), dict(par=dict(first=n + 1)),
           dict(nsamples=1 << 60), dict(fmt=(4, 1.0)), dict(fmt=(V.IQ_CU8, 0.0)), dict(fmt=(V.IQ_CS8, nan)),
           dict(fmt=(V.IQ_CS16, 2.0 ** 17))]
    for kw in bad:
        assert call(**kw) == 1, kw
        assert "bad arguments" in V.last_error(), kw
    assert call(nperiods=0) == 0
    torch.cuda.synchronize()
    assert bool((d_so == 7).all()) and bool((d_info == 7).all()) and bool((d_pw == 7).all())
    # what is allowed: no d_info, no d_power, first = nsamples, no samples at all, an integer format at 4 bytes, any thr
    # that is finite, more periods than the stream holds, a scale that F32 ignores
    assert call() == 0 and call(info=None) == 0 and call(pw=None) == 0 and call(info=None, pw=None) == 0
    assert call(par=dict(first=n)) == 0 and call(nsamples=0) == 0 and call(par=dict(thr=3.0e38)) == 0
    assert call(iq=P(d_iq, 4), fmt=(V.IQ_CS8, 1.0)) == 0 and call(fmt=(V.IQ_F32, nan)) == 0
    assert call(par=dict(B=512, null_blocks=4096, ref_blocks=4096, period_blocks=0xFFFFFFFF), nperiods=4) == 0
    torch.cuda.synchronize()
    assert d_so.tolist() == [-1] * 4
    with pytest.raises(ValueError):
        V.ofdm_acquire_dev(d_iq, 8, 4, 2, 100, 0.5, 2, d_so.to(torch.int32))
    with pytest.raises(ValueError):
        V.ofdm_acquire_dev(d_iq, 8, 4, 2, 100, 0.5, 2, d_so, d_info=d_info[:7])
    with pytest.raises(ValueError):
        V.ofdm_acquire_dev(d_iq, 8, 4, 2, 100, 0.5, 2, d_so, d_power=d_pw[:100])
    with pytest.raises(ValueError):
        V.ofdm_acquire_dev(d_iq, 8, 4, 2, 100, 0.5, 2, d_so, nsamples=n + 5)
    return len(bad)


def test_acquire_call_fails_loudly(V):
    """without a device: VIT_ERR_NO_DEVICE first, whatever the arguments, and an error text naming gfx950 - nothing is
    launched; with one, every argument rule is VIT_ERR_ARG"""
    import torch
    if torch.cuda.is_available():
        assert argument_error_cases(V, torch) >= 30
        return
    par = V.AcqParams(32, 64, 32, 6144, 1.0, 0, 0, 0)
    bad = V.AcqParams(3, 0, 0, 0, -1.0, 9, 5, 0)
    for p in (C.byref(par), C.byref(bad), None):
        assert V.lib().vit_ofdm_acquire_dev(None, 0, None, p, 1, None, None, None, None) == 2
        assert "gfx950" in V.last_error()
    assert V.lib().vit_ofdm_acquire_dev(None, 100, C.byref(V.IqFormat(9, 0.0)), None, -1, None, None, None, None) == 2
