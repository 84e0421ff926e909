#!/usr/bin/env python3
"""From the coarse start: what vit_ofdm_sync_dev costs against what a caller does today.  Mode I (nfft 2048, guard 504, null
symbol 2656: 196608 samples a frame), W = 64, M = 16, nco_bits 12, 512 frames and 4096 frames (6.4 GB of samples, far
past the Infinity Cache); 4 distinct frames from the time-domain transmitter (14 dB, an echo, per-frame offsets), tiled.
HIP-event times, the variants of one comparison alternating, every sample a window of at least 0.1 s, median of the
samples with min and max for the spread:
  - the call with cp_symbols = 75 (every guard of the frame) and with cp_symbols = 8;
  - today's estimator: the same algorithm in torch tensor ops (strided views of the guards, torch.angle, a tensor multiply
    by the fractional phasor, torch.fft, 33 rolled correlations, argmax, an inverse FFT, a threshold) ending in the same
    two device tables, at both cp_symbols;
  - a device-to-device copy that reads the bytes the call reads, nframes*(2*cp_symbols*(G-2W) + nfft)*8 (and writes as many);
  - vit_ofdm_demod_dev with rotation on the same frames, reading the tables the call wrote.
Parity: every output word of the first and last frames equals the numpy model of tests/test_sync_host.py; how many starts
and integer offsets of the torch estimator differ from the call's is counted, not asserted (its arithmetic is its own).
The kernel's own time comes from a separate rocprofv3 run of `bench_sync.py profile` (profiles/r11_sync_kstats.csv).

usage: bench_sync.py [samples | profile]"""
import json
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import _vitpkg  # noqa: E402
from test_ofdm_host import MODE_I  # noqa: E402
from test_sync_host import Params, prs_table, sync_model, transmit_frames  # noqa: E402

V = _vitpkg.load_package()
assert V.initialize() and V.device_count() >= 1, V.last_error()
profile = len(sys.argv) > 1 and sys.argv[1] == "profile"
samples = int(sys.argv[1]) if len(sys.argv) > 1 and not profile else 9
rng = np.random.default_rng(2031)
NFFT, K, NSYMS, FIC_SYMS, CIFS = MODE_I
G, NULL, SS, FS = 504, 2656, 2552, 196608
W, M, NCO_BITS, THR, BACKOFF, BASE = 64, 16, 12, 0.5, 100, 4
bins = V.freq_interleave_bins(NFFT)
d_bins = torch.from_numpy(bins.view(np.int16)).cuda()
tw, nco = V.fft_twiddles(NFFT), V.nco_table(NCO_BITS)
d_tw, d_nco = torch.from_numpy(tw).cuda(), torch.from_numpy(nco).cuda()
prs = prs_table(rng, NFFT, bins)
d_prs = torch.from_numpy(prs).cuda()
offsets = np.array([-7.3, 0.2, 4.45, 11.8])
prm0 = Params(NFFT, G, NSYMS, W, M, thr=THR, backoff=BACKOFF)
base, true, _ = transmit_frames(rng, prm0, prs, bins, BASE, offsets, lead=[NULL] * BASE, tail=[0] * BASE,
                                echo=(0.5 * np.exp(1.0j), 40), snr_db=14.0)
assert base.size == BASE * FS and (np.diff(true) == FS).all()
DELTA = 37  # the coarse start's error, the same for every frame (a table could differ per frame)
FIRST = int(true[0]) + DELTA
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
    return {"ms": round(ms, 4), "ms_min_max": [round(min(t), 4), round(max(t), 4)]}


def read_bytes(n, cp):
    return n * (2 * cp * (G - 2 * W) + NFFT) * 8


def tables(n):
    return (torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros((n, 2), dtype=torch.int32, device="cuda"),
            torch.zeros((n, 8), dtype=torch.int32, device="cuda"))


def call(d_iq, n, cp, out):
    V.ofdm_sync_dev(d_iq, NFFT, NSYMS, n, d_tw, SS, d_nco, NCO_BITS, d_prs, out[0], out[1], W, M, cp_symbols=cp, thr=THR,
                    backoff=BACKOFF, frame_stride=FS, first_start=FIRST, d_info=out[2])


d_Pc = torch.view_as_complex(d_prs.view(NFFT, 2)) if d_prs.dtype == torch.float32 else d_prs
d_Rc = (d_Pc * torch.roll(d_Pc, 1).conj()).conj()
d_i = torch.arange(NFFT, device="cuda", dtype=torch.float32)
d_t = None


def today(d_iq, n, cp, out):
    """the same estimator in tensor ops, ending in the same two tables"""
    a = torch.as_strided(d_iq, (n, cp, G - 2 * W), (FS, SS, 1), FIRST + SS - G + W)
    b = torch.as_strided(d_iq, (n, cp, G - 2 * W), (FS, SS, 1), FIRST + SS - G + W + NFFT)
    turn = torch.angle((a.conj() * b).sum(dim=(1, 2))) / (2 * math.pi)
    win = torch.as_strided(d_iq, (n, NFFT), (FS, 1), FIRST - W)
    y = torch.fft.fft(win * torch.polar(torch.ones_like(turn)[:, None], (-2 * math.pi / NFFT) * turn[:, None] * d_i[None, :]), dim=-1)
    d = y * torch.roll(y, 1, dims=-1).conj()
    metric = torch.stack([(torch.roll(d, -m, dims=-1) * d_Rc).sum(dim=-1).abs() for m in range(-M, M + 1)], dim=1)
    mhat = metric.argmax(dim=1) - M
    idx = (torch.arange(NFFT, device="cuda")[None, :] + mhat[:, None]) % NFFT
    h = torch.fft.ifft(torch.gather(y, 1, idx) * d_Pc.conj(), dim=-1)[:, :2 * W + 1]
    p = h.real * h.real + h.imag * h.imag
    tau = (p >= THR * p.max(dim=1, keepdim=True).values).to(torch.int8).argmax(dim=1)
    out[0].copy_(FIRST + d_t[:n] * FS - W + tau - BACKOFF)
    step = torch.round(-(mhat + turn) * (2.0 ** 32 / NFFT)).to(torch.int64) & 0xFFFFFFFF
    out[1][:, 0] = 0
    out[1][:, 1] = torch.where(step >= 1 << 31, step - (1 << 32), step).to(torch.int32)


def demod(d_iq, n, d_start, d_rot, out):
    V.ofdm_demod_dev(d_iq, MODE_I, d_bins, 254.0, n, d_tw, SS, d_start=d_start, d_nco=d_nco, nco_bits=NCO_BITS, d_rot=d_rot,
                     d_fic=out[0], d_ring=out[1])


def stream_of(n):
    reps = (n + BASE - 1) // BASE
    d = torch.from_numpy(base.reshape(BASE, FS)).cuda().repeat(reps, 1)[:n].reshape(-1)
    return torch.cat([d, torch.zeros(PAD, dtype=d.dtype, device="cuda")])


if profile:  # for rocprofv3: the calls alone, a few launches
    n = 512
    d_iq = stream_of(n)
    out = tables(n)
    soft = (torch.zeros((n, FIC_SYMS * 2 * K), dtype=torch.uint8, device="cuda"), torch.zeros((n * CIFS, 55296), dtype=torch.uint8, device="cuda"))
    for _ in range(5):
        call(d_iq, n, 75, out)
        call(d_iq, n, 8, out)
        demod(d_iq, n, out[0], out[1], soft)
    torch.cuda.synchronize()
    sys.exit(0)

result = {"shape": list(MODE_I), "sym_stride": SS, "frame_stride": FS, "W": W, "M": M, "nco_bits": NCO_BITS, "thr": THR,
          "sizes": {}}
ok_all = True
for n in (512, 4096):
    d_iq = stream_of(n)
    d_t = torch.arange(n, device="cuda", dtype=torch.int64)
    outs = [tables(n) for _ in range(4)]
    soft = (torch.zeros((n, FIC_SYMS * 2 * K), dtype=torch.uint8, device="cuda"), torch.zeros((n * CIFS, 55296), dtype=torch.uint8, device="cuda"))
    src75 = torch.empty(read_bytes(n, 75), dtype=torch.uint8, device="cuda")
    src8 = torch.empty(read_bytes(n, 8), dtype=torch.uint8, device="cuda")
    dst75, dst8 = torch.empty_like(src75), torch.empty_like(src8)
    call(d_iq, n, 75, outs[0])
    res = alternate([lambda: call(d_iq, n, 75, outs[0]), lambda: today(d_iq, n, 75, outs[1]),
                     lambda: call(d_iq, n, 8, outs[2]), lambda: today(d_iq, n, 8, outs[3]),
                     lambda: dst75.copy_(src75), lambda: dst8.copy_(src8),
                     lambda: demod(d_iq, n, outs[0][0], outs[0][1], soft)])
    torch.cuda.synchronize()
    head = min(n, 2)  # parity of the first and the last frames against the model
    par = True
    for sl in (slice(0, head), slice(n - head, n)):
        x = d_iq[sl.start * FS:sl.stop * FS + PAD].cpu().numpy()  # the frames' samples and what follows them
        coarse = FIRST + np.arange(head) * FS
        for o, cp in ((outs[0], 75), (outs[2], 8)):
            want = sync_model(x, coarse, Params(NFFT, G, NSYMS, W, M, cp_symbols=cp, thr=THR, backoff=BACKOFF), prs, tw, nco, NCO_BITS)
            par = par and np.array_equal(o[0][sl].cpu().numpy() - sl.start * FS, want[0])
            par = par and np.array_equal(o[1][sl].cpu().numpy().view(np.uint32), want[1])
            par = par and np.array_equal(o[2][sl].cpu().numpy().view(np.uint32), want[2])
    want_start = torch.from_numpy(np.tile(true, (n + BASE - 1) // BASE)[:n] - BACKOFF).cuda() + (d_t // BASE) * (BASE * FS)
    right = [int((o[0] == want_start).sum()) for o in outs]
    differ = [[int((outs[a][0] != outs[b][0]).sum()), int(((outs[a][1][:, 1] - outs[b][1][:, 1]).abs() > (1 << 32) // NFFT // 2).sum())]
              for a, b in ((0, 1), (2, 3))]
    spread = max(max(t) - min(t) for _, t in res[:4])
    faster = bool(res[1][0] - res[0][0] > spread and res[3][0] - res[2][0] > spread)
    result["sizes"][str(n)] = {
        "nframes": n, "sample_bytes": n * FS * 8, "read_bytes_cp75": read_bytes(n, 75), "read_bytes_cp8": read_bytes(n, 8),
        "ofdm_sync_cp75": dict(stat(res[0]), read_tb_per_s=round(read_bytes(n, 75) / (res[0][0] * 1e-3) / 1e12, 3), us_per_frame=round(res[0][0] * 1e3 / n, 4)),
        "torch_estimator_cp75": stat(res[1]),
        "ofdm_sync_cp8": dict(stat(res[2]), read_tb_per_s=round(read_bytes(n, 8) / (res[2][0] * 1e-3) / 1e12, 3), us_per_frame=round(res[2][0] * 1e3 / n, 4)),
        "torch_estimator_cp8": stat(res[3]),
        "copy_read_bytes_cp75": dict(stat(res[4]), read_tb_per_s=round(read_bytes(n, 75) / (res[4][0] * 1e-3) / 1e12, 3)),
        "copy_read_bytes_cp8": dict(stat(res[5]), read_tb_per_s=round(read_bytes(n, 8) / (res[5][0] * 1e-3) / 1e12, 3)),
        "ofdm_demod_rotating": stat(res[6]),
        "speedup_over_torch_cp75": round(res[1][0] / res[0][0], 3), "speedup_over_torch_cp8": round(res[3][0] / res[2][0], 3),
        "ratio_to_copy_cp75": round(res[0][0] / res[4][0], 3), "ratio_to_copy_cp8": round(res[2][0] / res[5][0], 3),
        "ratio_to_demod_cp75": round(res[0][0] / res[6][0], 3), "ratio_to_demod_cp8": round(res[2][0] / res[6][0], 3),
        "starts_on_the_first_path": {"sync_cp75": right[0], "torch_cp75": right[1], "sync_cp8": right[2], "torch_cp8": right[3]},
        "torch_differs_in_starts_and_offsets": differ,
        "faster_than_torch_by_more_than_the_spread": faster, "spread_ms": round(spread, 4), "parity_ok": bool(par)}
    ok_all = ok_all and par and faster
    del d_iq, outs, soft, src75, src8, dst75, dst8
print(json.dumps(result))
sys.exit(0 if ok_all else 1)
