#!/usr/bin/env python3
"""Integer sample formats: what the *_iq_dev calls cost against the float32 path and against what a caller does today.
Mode I (nfft 2048, guard 504, null symbol 2656: 196608 samples a frame), W = 64, M = 16, nco_bits 12, 512 frames and 4096
frames (6.4 GB as float32); 4 distinct frames from the time-domain transmitter of tests/tools/bench_sync.py, rounded to
each format at 90 % of full range, tiled.  The method is bench_sync.py's: HIP-event times, the variants of one comparison
alternating, every sample a window of at least 0.1 s, 9 samples, the median with min and max for the spread.  Per format
(cu8, cs8, cs16) and per kernel (vit_ofdm_demod_dev with rotation, vit_ofdm_sync_dev at cp_symbols 75 and 8):
  (a) the *_iq_dev call on the raw samples;
  (b) the existing float32 call on floats converted beforehand - the float path as it was;
  (c) a conversion in torch tensor ops into a float32 buffer, then the float32 call;
  (d) vit_iq_convert_dev into that buffer, then the float32 call.
Per case the tool says whether (a) is slower than (b) by more than the larger of the two variants' spreads (max - min),
and whether (a) beats (c) and (d).  Parity: the outputs of (a) equal those of (b) bit for bit.  It also records the device
bytes the stream holds, raw against float32.

usage: bench_iqfmt.py [samples]"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import _vitpkg  # noqa: E402
from test_iqfmt_host import DTYPES, INT_FORMATS, quantise  # noqa: E402
from test_ofdm_host import MODE_I  # noqa: E402
from test_sync_host import Params, prs_table, transmit_frames  # noqa: E402

V = _vitpkg.load_package()
assert V.initialize() and V.device_count() >= 1, V.last_error()
samples = int(sys.argv[1]) if len(sys.argv) > 1 else 9
rng = np.random.default_rng(2033)
NFFT, K, NSYMS, FIC_SYMS, CIFS = MODE_I
G, NULL, SS, FS = 504, 2656, 2552, 196608
W, M, NCO_BITS, THR, BACKOFF, BASE = 64, 16, 12, 0.5, 100, 4
NAMES = {V.IQ_CU8: "cu8", V.IQ_CS8: "cs8", V.IQ_CS16: "cs16"}
bins = V.freq_interleave_bins(NFFT)
d_bins = torch.from_numpy(bins.view(np.int16)).cuda()
d_tw, d_nco = torch.from_numpy(V.fft_twiddles(NFFT)).cuda(), torch.from_numpy(V.nco_table(NCO_BITS)).cuda()
prs = prs_table(rng, NFFT, bins)
d_prs = torch.from_numpy(prs).cuda()
base, true, _ = transmit_frames(rng, Params(NFFT, G, NSYMS, W, M, thr=THR, backoff=BACKOFF), prs, bins, BASE,
                                np.array([-7.3, 0.2, 4.45, 11.8]), lead=[NULL] * BASE, tail=[0] * BASE,
                                echo=(0.5 * np.exp(1.0j), 40), snr_db=14.0)
assert base.size == BASE * FS and (np.diff(true) == FS).all()
FIRST = int(true[0]) + 37  # the coarse start's error, the same for every frame
PAD = 4 * W


def sample(fn, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / k


def alternate(fns, warm=3):
    """median ms of each fn and its samples, the fns alternating; each sample repeats its fn for at least 0.1 s"""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ks = [max(2, int(np.ceil(100.0 / max(sample(fn, 2), 1e-3)))) for fn in fns]
    ts = [[] for _ in fns]
    for _ in range(samples):
        for t, fn, k in zip(ts, fns, ks):
            t.append(sample(fn, k))
    return [(float(np.median(t)), t) for t in ts]


def stat(ms_t):
    ms, t = ms_t
    return {"ms": round(ms, 4), "ms_min_max": [round(min(t), 4), round(max(t), 4)], "spread_ms": round(max(t) - min(t), 4)}


def tables(n):
    return (torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros((n, 2), dtype=torch.int32, device="cuda"),
            torch.zeros((n, 8), dtype=torch.int32, device="cuda"))


def soft(n):
    return (torch.zeros((n, FIC_SYMS * 2 * K), dtype=torch.uint8, device="cuda"),
            torch.zeros((n * CIFS, 55296), dtype=torch.uint8, device="cuda"))


def sync(d_iq, n, cp, out, **fmt):
    V.ofdm_sync_dev(d_iq, NFFT, NSYMS, n, d_tw, SS, d_nco, NCO_BITS, d_prs, out[0], out[1], W, M, cp_symbols=cp, thr=THR,
                    backoff=BACKOFF, frame_stride=FS, first_start=FIRST, d_info=out[2], **fmt)


def demod(d_iq, n, tab, out, **fmt):
    V.ofdm_demod_dev(d_iq, MODE_I, d_bins, 254.0, n, d_tw, SS, d_start=tab[0], d_nco=d_nco, nco_bits=NCO_BITS, d_rot=tab[1],
                     d_fic=out[0], d_ring=out[1], **fmt)


def torch_convert(d_raw, fmt, scale, d_flt):
    """what a caller writes today: cast, offset and scale in tensor ops, into a float32 buffer"""
    if fmt == V.IQ_CU8:
        torch.sub(d_raw, 127.5, out=d_flt)
        d_flt.mul_(2.0 * scale)
    else:
        torch.mul(d_raw, scale, out=d_flt)


def stream_of(raw_base, n):
    reps = (n + BASE - 1) // BASE
    d = torch.from_numpy(raw_base.reshape(BASE, 2 * FS)).cuda().repeat(reps, 1)[:n].reshape(-1)
    return torch.cat([d, torch.zeros(2 * PAD, dtype=d.dtype, device="cuda")])


def compare(a, b, c, d):
    """(a) against the float path (b) and against today's (c), (d): each a (median, samples) pair"""
    spread = max(max(a[1]) - min(a[1]), max(b[1]) - min(b[1]))
    return {"iq_call": stat(a), "float_call_on_converted_floats": stat(b), "torch_convert_then_float_call": stat(c),
            "iq_convert_then_float_call": stat(d), "iq_over_float": round(a[0] / b[0], 4),
            "allowed_spread_ms": round(spread, 4), "iq_minus_float_ms": round(a[0] - b[0], 4),
            "iq_slower_than_float_by_more_than_the_spread": bool(a[0] - b[0] > spread),
            "iq_faster_than_float_by_more_than_the_spread": bool(b[0] - a[0] > spread),
            "iq_beats_torch_convert": bool(a[0] < c[0]), "iq_beats_iq_convert": bool(a[0] < d[0])}


result = {"shape": list(MODE_I), "sym_stride": SS, "frame_stride": FS, "W": W, "M": M, "nco_bits": NCO_BITS, "samples": samples,
          "sizes": {}}
parity = True
for n in (512, 4096):
    size = {"nframes": n, "formats": {}}
    for fmt in INT_FORMATS:
        raw_base, scale = quantise(base, fmt)
        assert raw_base.dtype == DTYPES[fmt]
        f = dict(iq_format=fmt, iq_scale=scale)
        d_raw = stream_of(raw_base, n)
        d_pre = torch.empty(d_raw.numel(), dtype=torch.float32, device="cuda")  # (b): converted beforehand
        d_work = torch.empty_like(d_pre)                                        # (c), (d): converted in the timed window
        V.iq_convert_dev(d_raw, fmt, scale, d_pre)
        tab = tables(n)
        sync(d_pre, n, 75, tab)  # the tables the demodulator reads
        o_dem = [soft(n) for _ in range(2)]
        o_syn = [tables(n) for _ in range(4)]
        entry = {"scale": scale, "stream_bytes_raw": d_raw.numel() * d_raw.element_size(), "stream_bytes_float32": d_pre.numel() * 4}

        def then(convert, call):
            def run():
                convert()
                call()
            return run

        def by_torch():
            torch_convert(d_raw, fmt, scale, d_work)

        def by_lib():
            V.iq_convert_dev(d_raw, fmt, scale, d_work)

        res = alternate([lambda: demod(d_raw, n, tab, o_dem[0], **f), lambda: demod(d_pre, n, tab, o_dem[1]),
                         then(by_torch, lambda: demod(d_work, n, tab, o_dem[1])), then(by_lib, lambda: demod(d_work, n, tab, o_dem[1]))])
        entry["ofdm_demod_rotating"] = compare(*res)
        for cp, (oa, ob) in ((75, o_syn[:2]), (8, o_syn[2:])):
            res = alternate([lambda: sync(d_raw, n, cp, oa, **f), lambda: sync(d_pre, n, cp, ob),
                             then(by_torch, lambda: sync(d_work, n, cp, ob)), then(by_lib, lambda: sync(d_work, n, cp, ob))])
            entry["ofdm_sync_cp%d" % cp] = compare(*res)
        res = alternate([by_torch, by_lib])
        entry["torch_convert_alone"], entry["iq_convert_alone"] = stat(res[0]), stat(res[1])
        torch.cuda.synchronize()
        same = all(torch.equal(p, q) for p, q in zip(o_dem[0] + o_syn[0] + o_syn[2], o_dem[1] + o_syn[1] + o_syn[3]))
        same = same and torch.equal(d_work, d_pre) and bool((o_dem[0][0] != 0).any()) and bool((o_syn[0][0] > 0).all())
        entry["parity_ok"] = bool(same)
        parity = parity and same
        size["formats"][NAMES[fmt]] = entry
        del d_raw, d_pre, d_work, o_dem, o_syn, tab
    result["sizes"][str(n)] = size
result["parity_ok"] = bool(parity)
print(json.dumps(result))
sys.exit(0 if parity else 1)
