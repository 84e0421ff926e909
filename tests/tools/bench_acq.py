#!/usr/bin/env python3
"""From the stream: what vit_ofdm_acquire_dev costs against what a caller does today.  Mode I (nfft 2048, guard 504, null
symbol 2656: 196608 samples a frame period), B 32, Ln 64, Lr 32, Pb 6144, at 512 and 4096 periods (4096 periods of float32
are 6.4 GB of samples, far past the Infinity Cache), in float32 and in CU8; 4 distinct frames from the time-domain
transmitter (10 dB), tiled.  HIP-event times, the variants of one comparison alternating, every sample a window of at least
0.1 s, median of the samples with min and max for the spread:
  - the call (both kernels, powers in the library's own buffer);
  - the block-power pass: the call with d_power given and ONE period, so all nblk powers are written and the search is one
    workgroup (its microseconds are inside this figure); the search pass is the call minus this;
  - a device-to-device copy of the bytes the call reads (it writes as many);
  - today's estimator: the same search in torch tensor ops (block sums, a float64 cumulative sum for the windows, a
    division, argmin per period), ending in the same device table;
  - vit_ofdm_sync_dev (75 guards) on the same frames, float32.
The one condition: on float32 at 4096 periods the block-power pass reads what the copy reads and writes next to nothing, so
it must not take longer than the copy by more than the spread of the two measurements.  Everything else is recorded.
Parity: every output word of the first and last two periods equals the numpy model of tests/test_acq_host.py.
The two pass figures above are call-time differences.  The kernels' own times come from separate `rocprofv3 --kernel-trace
--stats` runs of `bench_acq.py profile [nperiods]` (profiles/r15_acq_kstats_512.csv, profiles/r15_acq_kstats_4096.csv).

usage: bench_acq.py [samples | profile [nperiods]] [--out FILE]   (FILE defaults to profiles/r15_acq_bench.json)"""
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
from test_acq_host import Acq, acquire_model  # noqa: E402
from test_iqfmt_host import IQ_CU8, convert_model, quantise  # noqa: E402
from test_ofdm_host import MODE_I  # noqa: E402
from test_sync_host import Params, prs_table, transmit_frames  # noqa: E402

V = _vitpkg.load_package()
assert V.initialize() and V.device_count() >= 1, V.last_error()
args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "r15_acq_bench.json")
if "--out" in args:
    out_path = args[args.index("--out") + 1]
    del args[args.index("--out"):args.index("--out") + 2]
profile = bool(args) and args[0] == "profile"
samples = int(args[0]) if args and not profile else 9
rng = np.random.default_rng(2035)
NFFT, K, NSYMS, FIC_SYMS, CIFS = MODE_I
G, NULL, SS, FS = 504, 2656, 2552, 196608
B, LN, LR, PB, BASE = 32, 64, 32, 6144, 4
W, M, NCO_BITS, BACKOFF = 64, 16, 12, 0
ACQ = Acq(B, LN, LR, PB, thr=0.5 * LN / LR, offset=G + B // 2 - BACKOFF)
PAD = (LN + LR) * B  # behind the last frame: its period is whole, and vit_ofdm_sync_dev's last window fits
assert PB * B == FS
bins = V.freq_interleave_bins(NFFT)
tw, nco = V.fft_twiddles(NFFT), V.nco_table(NCO_BITS)
d_tw, d_nco = torch.from_numpy(tw).cuda(), torch.from_numpy(nco).cuda()
prs = prs_table(rng, NFFT, bins)
d_prs = torch.from_numpy(prs).cuda()
base, true, _ = transmit_frames(rng, Params(NFFT, G, NSYMS, W, M), prs, bins, BASE, [0.0] * BASE, lead=[NULL] * BASE, tail=[0] * BASE,
                                snr_db=10.0)
assert base.size == BASE * FS and (np.diff(true) == FS).all()
raw8, SCALE8 = quantise(base, IQ_CU8)
FORMATS = {"f32": (V.IQ_F32, 1.0, 8), "cu8": (IQ_CU8, SCALE8, 2)}


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


def stat(ms_t, nbytes=None):
    ms, t = ms_t
    d = {"ms": round(ms, 4), "ms_min_max": [round(min(t), 4), round(max(t), 4)]}
    if nbytes is not None:
        d["read_tb_per_s"] = round(nbytes / (ms * 1e-3) / 1e12, 3)
    return d


def stream_of(name, n):
    """n periods of the format and PAD samples of the first frame's null behind them"""
    host = base if name == "f32" else raw8
    d = torch.from_numpy(host.reshape((BASE, FS) + host.shape[1:])).cuda()
    d = d.repeat((-(-n // BASE),) + (1,) * (d.dim() - 1))[:n].reshape((n * FS,) + host.shape[1:])
    return torch.cat([d, d[:PAD]]).reshape(-1)


def call(name, d_iq, n, out, d_power=None):
    fmt, scale, _ = FORMATS[name]
    V.ofdm_acquire_dev(d_iq, B, LN, LR, PB, ACQ.thr, n, out[0], offset=ACQ.offset, d_info=out[1], d_power=d_power, iq_format=fmt,
                       iq_scale=scale)


def today(name, d_iq, n, out):
    """the same search in tensor ops, ending in the same table"""
    if name == "f32":
        v = torch.view_as_real(d_iq) if d_iq.is_complex() else d_iq.view(-1, 2)
    else:
        v = (d_iq.view(-1, 2).to(torch.float32) * 2.0 - 255.0) * SCALE8
    p = (v * v).sum(dim=1).view(-1, B).sum(dim=1)
    cs = torch.cat([torch.zeros(1, dtype=torch.float64, device="cuda"), torch.cumsum(p.to(torch.float64), 0)])
    j = n * PB
    N = (cs[LN:LN + j] - cs[0:j]).to(torch.float32)
    R = (cs[LN + LR:LN + LR + j] - cs[LN:LN + j]).to(torch.float32)
    q = torch.where(R > 0, N / R, torch.full_like(R, float("inf"))).view(n, PB)
    qmin, i = q.min(dim=1)
    start = (LN + torch.arange(n, device="cuda") * PB + i) * B + ACQ.offset
    out[0].copy_(torch.where(qmin <= ACQ.thr, start, torch.full_like(start, -1)))


def sync(d_iq, n, out):
    V.ofdm_sync_dev(d_iq, NFFT, NSYMS, n, d_tw, SS, d_nco, NCO_BITS, d_prs, out[0], out[1], W, M, frame_stride=FS,
                    first_start=int(true[0]))


def tables(n):
    return torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros((n, 4), dtype=torch.int32, device="cuda")


if profile:  # for rocprofv3: the calls alone, a few launches; `profile 4096` for the large size
    n = int(args[1]) if len(args) > 1 else 512
    for name in FORMATS:
        d_iq = stream_of(name, n)
        out = tables(n)
        for _ in range(5):
            call(name, d_iq, n, out)
    torch.cuda.synchronize()
    sys.exit(0)

result = {"shape": list(MODE_I), "frame_period": FS, "B": B, "null_blocks": LN, "ref_blocks": LR, "period_blocks": PB,
          "thr": ACQ.thr, "sizes": {}}
ok_all = True
for n in (512, 4096):
    entry = {"nperiods": n}
    for name, (fmt, scale, sb) in FORMATS.items():
        d_iq = stream_of(name, n)
        nbytes = (n * FS + PAD) * sb
        nblk = (n * FS + PAD) // B
        out, out1, out_t = tables(n), tables(1), tables(n)
        d_power = torch.zeros(nblk, dtype=torch.float32, device="cuda")
        src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        fns = [lambda: call(name, d_iq, n, out), lambda: call(name, d_iq, 1, out1, d_power), lambda: dst.copy_(src),
               lambda: today(name, d_iq, n, out_t)]
        if name == "f32":
            so = (torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros((n, 2), dtype=torch.int32, device="cuda"))
            fns.append(lambda: sync(d_iq, n, so))
        res = alternate(fns)
        torch.cuda.synchronize()
        par = True  # parity of the first and the last two periods against the model
        host = d_iq.view(-1, 2) if name != "f32" else d_iq
        for lo in (0, n - 2):
            x = host[lo * FS:(lo + 2) * FS + PAD].cpu().numpy()
            x = x if name == "f32" else convert_model(x, fmt, scale)
            start, info, p = acquire_model(x, ACQ, 2)
            par = par and np.array_equal(out[0][lo:lo + 2].cpu().numpy(), np.where(start >= 0, start + lo * FS, -1))
            par = par and np.array_equal(out[1][lo:lo + 2].cpu().numpy().view(np.uint32), info)
            par = par and np.array_equal(d_power[lo * PB:lo * PB + p.size].cpu().numpy().view(np.uint32), p.view(np.uint32))
        want = torch.from_numpy(np.tile(true - G, -(-n // BASE))[:n]).cuda() + (torch.arange(n, device="cuda") // BASE) * (BASE * FS)
        err = out[0] - ACQ.offset - want  # the found block's first sample against the edge
        spread = max(max(t) - min(t) for _, t in res[1:3])
        e = {"read_bytes": nbytes,
             "acquire": dict(stat(res[0], nbytes), us_per_period=round(res[0][0] * 1e3 / n, 4)),
             "block_power_pass": stat(res[1], nbytes), "search_pass_ms": round(res[0][0] - res[1][0], 4),
             "copy_of_the_bytes_read": stat(res[2], nbytes), "torch_estimator": stat(res[3]),
             "ratio_power_pass_to_copy": round(res[1][0] / res[2][0], 3), "spread_ms": round(spread, 4),
             "speedup_over_torch": round(res[3][0] / res[0][0], 3),
             "accepted": int((out[0] >= 0).sum()), "edge_minus_block_start_min_max": [int(-err.max()), int(-err.min())],
             "torch_differs_in_starts": int((out[0] != out_t[0]).sum()), "parity_ok": bool(par)}
        if name == "f32":
            e["ofdm_sync_cp75"] = stat(res[4])
            e["ratio_to_sync"] = round(res[0][0] / res[4][0], 3)
            if n == 4096:
                e["power_pass_no_slower_than_copy"] = bool(res[1][0] <= res[2][0] + spread)
                ok_all = ok_all and e["power_pass_no_slower_than_copy"]
        ok_all = ok_all and par
        entry[name] = e
        del d_iq, d_power, src, dst, out, out_t
    result["sizes"][str(n)] = entry
text = json.dumps(result)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text + "\n")
print(text)
sys.exit(0 if ok_all else 1)
