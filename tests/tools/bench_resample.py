#!/usr/bin/env python3
"""Before the stream: what vit_iq_resample_dev costs against what a caller does today.  Three inputs, each of 512 and 4096
mode-I frame periods (96 ms each):
  - 2.5 MS/s (240000 samples a period) in CU8 and in float32: 512/625, 32 taps a phase, one channel, rotation on - the
    stream of tests/test_resample_host.py's whole-chain case, its three periods tiled;
  - 10 MS/s (960000 samples a period) in CS16: 128/625, 128 taps a phase, 5 channels at multiples of 1.712 MHz - noise.
HIP-event times, the variants of one comparison alternating, every sample a window of at least 0.1 s, median of the samples
with min and max for the spread:
  - the call;
  - with --ab LIB the same call in a second build of the library (the taps read through the cache instead of LDS:
    build(extra=["-DVIT_RESAMPLE_TAPS_LDS=0"], out=LIB)), its outputs compared with the product's in every bit;
  - a device-to-device copy of as many bytes as the call reads plus writes;
  - today's resampler: the same result from torch tensor ops - convert, multiply by the phasor, then the polyphase filter
    as a gather of every output's T samples and its row of taps, 2^20 outputs at a time (at 4096 periods of the 10 MS/s
    input one such call takes seconds and is left out: the 512-period figure stands for it);
  - vit_ofdm_acquire_dev + vit_ofdm_sync_dev + vit_ofdm_demod_dev on the call's output (one channel), which the call's time
    is given as a share of; for the 5-channel input the share is against 5 such chains.
Nothing is asserted about speed.  Parity: the first and the last 2048 outputs of every channel equal the numpy model of
tests/test_resample_host.py in every bit, and the torch result agrees with the call to 1e-4 of the largest output.

usage: bench_resample.py [samples] [--ab LIB] [--sizes 512,4096] [--out FILE]   (FILE defaults to profiles/r17_resample_bench.json)"""
import ctypes as C
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
from test_iqfmt_host import IQ_CS16, IQ_CU8, convert_model, quantise  # noqa: E402
from test_ofdm_host import MODE_I  # noqa: E402
from test_resample_host import CHAIN_CUTOFF, Rs, chain_case, out_count_model, resample_model  # noqa: E402
from test_sync_host import prs_table  # noqa: E402

V = _vitpkg.load_package()
O = _vitpkg.load_oracle()
assert V.initialize() and V.device_count() >= 1, V.last_error()
args = sys.argv[1:]


def option(name, default):
    if name not in args:
        return default
    i = args.index(name)
    value = args[i + 1]
    del args[i:i + 2]
    return value


out_path = option("--out", os.path.join(ROOT, "profiles", "r17_resample_bench.json"))
ab_path = option("--ab", None)
sizes = [int(v) for v in option("--sizes", "512,4096").split(",")]
samples = int(args[0]) if args else 9
NFFT, K, NSYMS = MODE_I[:3]
G, SS, FS, NCO_BITS = 504, 2552, 196608, 12
B, LN, LR, PB, W, M_SYNC = 32, 64, 32, 6144, 64, 2
CHUNK = 1 << 20
nco = V.nco_table(NCO_BITS)
d_nco = torch.from_numpy(nco).cuda()
d_nco_c = torch.view_as_complex(d_nco)
d_tw = torch.from_numpy(V.fft_twiddles(NFFT)).cuda()
bins = V.freq_interleave_bins(NFFT)
d_bins = torch.from_numpy(bins.view(np.int16)).cuda()
d_prs = torch.from_numpy(prs_table(np.random.default_rng(17), NFFT, bins)).cuda()
AB = None
if ab_path:
    AB = C.CDLL(ab_path)
    AB.vit_iq_resample_dev.argtypes = V.lib().vit_iq_resample_dev.argtypes


def step_of(f_hz, fs):
    return int(round(-f_hz / fs * 2.0 ** 32)) % (1 << 32)


def inputs():
    """name -> (period samples at the input rate, host samples of some whole periods in the device's format, format, scale,
    bytes a sample, Rs)"""
    x = chain_case(O)[0][:3 * 240000]
    raw8, s8 = quantise(x, IQ_CU8)
    r25 = Rs(512, 625, V.resample_taps(512, 32, CHAIN_CUTOFF), rot=[(0, step_of(200.0e3, 2.5e6))], nco_bits=NCO_BITS)
    rng = np.random.default_rng(10)
    n10 = 2 * 960000
    raw16, s16 = quantise(rng.standard_normal(n10) + 1j * rng.standard_normal(n10), IQ_CS16, fill=0.5)
    rot = [(0, step_of(k * 1.712e6, 10.0e6)) for k in (-2, -1, 0, 1, 2)]
    r10 = Rs(128, 625, V.resample_taps(128, 128, 1.024e6 / 10.0e6), rot=rot, nco_bits=NCO_BITS)
    return {"2.5MS/s cu8": (240000, raw8, IQ_CU8, s8, 2, r25), "2.5MS/s f32": (240000, x, V.IQ_F32, 1.0, 8, r25),
            "10MS/s cs16 x5": (960000, raw16, IQ_CS16, s16, 4, r10)}


def sample(fn, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / k


def alternate(fns, warm=2):
    """median ms of each fn and its samples, the fns alternating; each sample repeats its fn for at least 0.1 s"""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ks = [max(1, int(np.ceil(100.0 / max(sample(fn, 1), 1e-3)))) for fn in fns]
    ts = [[] for _ in fns]
    for _ in range(samples):
        for t, fn, k in zip(ts, fns, ks):
            t.append(sample(fn, k))
    return [(float(np.median(t)), t) for t in ts]


def stat(ms_t, nbytes=None):
    ms, t = ms_t
    d = {"ms": round(ms, 4), "ms_min_max": [round(min(t), 4), round(max(t), 4)]}
    if nbytes is not None:
        d["tb_per_s"] = round(nbytes / (ms * 1e-3) / 1e12, 3)
    return d


def stream_of(host, period, n):
    """n periods and one more symbol of the host's periods, tiled on the device -> a flat tensor of the format's type"""
    have = host.shape[0] // period
    d = torch.from_numpy(np.ascontiguousarray(host[:have * period]).reshape((have, period) + host.shape[1:])).cuda()
    d = d.repeat((-(-(n + 1) // have),) + (1,) * (d.dim() - 1)).reshape((-1,) + host.shape[1:])[:n * period + 4096]
    return d.reshape(-1)


def raw_call(lib, d_iq, ns, fmt, scale, r, d_taps, nout, d_out):
    pairs = np.ascontiguousarray(r.rot, np.uint32)
    par = V.ResampleParams(r.L, r.M, r.T, r.nchan, r.pos0, d_taps.data_ptr(), d_nco.data_ptr(), r.nco_bits, 0, pairs.ctypes.data)
    f = None if fmt == V.IQ_F32 else C.byref(V.IqFormat(fmt, scale))
    rc = lib.vit_iq_resample_dev(C.c_void_p(d_iq.data_ptr()), ns, f, C.byref(par), nout, C.c_void_p(d_out.data_ptr()), nout,
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, V.last_error()


def today(d_iq, fmt, scale, r, d_taps, nout, out):
    """the same result in tensor ops: out (nchan, nout) complex64"""
    T = r.T
    k = torch.arange(T, device="cuda")
    for m0 in range(0, nout, CHUNK):
        m1 = min(m0 + CHUNK, nout)
        P = torch.arange(m0, m1, device="cuda", dtype=torch.int64) * r.M + r.pos0
        n0, phi = P // r.L, P % r.L
        lo, hi = (r.pos0 + m0 * r.M) // r.L, (r.pos0 + (m1 - 1) * r.M) // r.L + T
        if fmt == V.IQ_F32:
            x = d_iq[lo:hi]
        else:
            v = d_iq.view(-1, 2)[lo:hi].to(torch.float32)
            x = torch.view_as_complex(((v * 2.0 - 255.0) if fmt == IQ_CU8 else v) * scale)
        idx = (n0 - lo)[:, None] + k[None, :]
        g = d_taps[phi]
        n = torch.arange(lo, hi, device="cuda", dtype=torch.int64)
        for c in range(r.nchan):
            ph = (int(r.rot[c, 0]) + n * int(r.rot[c, 1])) & 0xFFFFFFFF
            y = x * d_nco_c[ph >> (32 - r.nco_bits)]
            out[c, m0:m1] = (y[idx] * g).sum(dim=1)


def chain(d_y, n, tables):
    d_start, d_rot, d_fic = tables
    V.ofdm_acquire_dev(d_y, B, LN, LR, PB, 0.5 * LN / LR, n, d_start, offset=G + 22)
    V.ofdm_sync_dev(d_y, NFFT, NSYMS, n, d_tw, SS, d_nco, NCO_BITS, d_prs, d_start, d_rot, W, M_SYNC, cp_symbols=4, backoff=252,
                    frame_stride=FS, first_start=4096)
    V.ofdm_demod_dev(d_y, MODE_I, d_bins, 254.0, n, d_tw, SS, d_start=d_start, d_nco=d_nco, nco_bits=NCO_BITS, d_rot=d_rot,
                     d_fic=d_fic)


result = {"samples": samples, "ab_library": os.path.basename(ab_path) if ab_path else None, "sizes": {}}
ok_all = True
for n in sizes:
    entry = {"nperiods": n}
    for name, (period, host, fmt, scale, sb, r) in inputs().items():
        d_iq = stream_of(host, period, n)
        ns = d_iq.numel() // 2 if fmt != V.IQ_F32 else d_iq.numel()
        nout = n * FS
        assert nout <= out_count_model(ns, r.L, r.M, r.T)
        d_taps = torch.from_numpy(r.taps).cuda()
        out = torch.zeros((r.nchan, nout), dtype=torch.complex64, device="cuda")
        nbytes = ((nout - 1) * r.M // r.L + r.T) * sb + r.nchan * nout * 8
        src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        with_torch = not (r.nchan > 1 and n > 512)
        fns = [lambda: raw_call(V.lib(), d_iq, ns, fmt, scale, r, d_taps, nout, out), lambda: dst.copy_(src)]
        names = ["call", "copy_of_the_bytes_read_and_written"]
        if AB is not None:
            out_ab = torch.zeros_like(out)
            fns.append(lambda: raw_call(AB, d_iq, ns, fmt, scale, r, d_taps, nout, out_ab))
            names.append("call_ab")
        if with_torch:
            out_t = torch.zeros_like(out)
            fns.append(lambda: today(d_iq, fmt, scale, r, d_taps, nout, out_t))
            names.append("torch_ops")
        res = dict(zip(names, alternate(fns)))
        del src, dst
        # parity: the ends of every channel against the model
        par = True
        for lo_m, hi_m in ((0, 2048), (nout - 2048, nout)):
            lo, hi = lo_m * r.M // r.L, ((hi_m - 1) * r.M) // r.L + r.T
            seg = (d_iq[lo:hi] if fmt == V.IQ_F32 else d_iq.view(-1, 2)[lo:hi]).cpu().numpy()
            seg = seg if fmt == V.IQ_F32 else convert_model(seg, fmt, scale)
            rot = np.stack([(r.rot[:, 0] + lo * r.rot[:, 1]) % (1 << 32), r.rot[:, 1]], axis=1)
            want = resample_model(seg, Rs(r.L, r.M, r.taps, lo_m * r.M - lo * r.L, rot, r.nco_bits), hi_m - lo_m)
            par = par and np.array_equal(out[:, lo_m:hi_m].cpu().numpy(), want)
        e = {"samples_in": ns, "outputs_per_channel": nout, "channels": r.nchan, "L": r.L, "M": r.M, "T": r.T,
             "bytes_read_and_written": nbytes, "call": stat(res["call"], nbytes),
             "copy_of_the_bytes_read_and_written": stat(res["copy_of_the_bytes_read_and_written"], nbytes),
             "ratio_call_to_copy": round(res["call"][0] / res["copy_of_the_bytes_read_and_written"][0], 3),
             "parity_ok": bool(par)}
        if AB is not None:
            e["call_ab"] = stat(res["call_ab"], nbytes)
            e["ratio_ab_to_call"] = round(res["call_ab"][0] / res["call"][0], 3)
            e["ab_equal_in_every_bit"] = bool(torch.equal(out.view(torch.int64), out_ab.view(torch.int64)))
            par = par and e["ab_equal_in_every_bit"]
            del out_ab
        if with_torch:
            e["torch_ops"] = stat(res["torch_ops"])
            e["speedup_over_torch"] = round(res["torch_ops"][0] / res["call"][0], 2)
            e["torch_max_error_over_max_output"] = float((out_t - out).abs().max() / out.abs().max())
            par = par and e["torch_max_error_over_max_output"] < 1e-4
            del out_t
        # the chain behind it on channel 0
        tables = (torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros((n, 2), dtype=torch.int32, device="cuda"),
                  torch.zeros((n, 3 * 2 * K), dtype=torch.uint8, device="cuda"))
        d_y = out[0]
        ch = alternate([lambda: chain(d_y, n - 1, tables)])[0]
        e["acquire_sync_demod_one_channel"] = stat(ch)
        e["call_share_of_the_chains"] = round(res["call"][0] / (r.nchan * ch[0]), 3)
        ok_all = ok_all and par
        entry[name] = e
        del d_iq, out, d_y, tables
        torch.cuda.empty_cache()
        print(name, n, json.dumps(e), flush=True)
    result["sizes"][str(n)] = entry
text = json.dumps(result)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text + "\n")
print(text)
sys.exit(0 if ok_all else 1)
