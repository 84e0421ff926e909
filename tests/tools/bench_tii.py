#!/usr/bin/env python3
"""Transmitter identification: what vit_ofdm_tii_dev costs against what a caller does today.  Mode I (nfft 2048, guard 504,
null symbol 2656: 196608 samples a frame period), the standard's pair table, navg 8, thr 2.5, at 512 and 4096 frames, in
float32 and in CU8, with the rotation; 4 distinct frames from the time-domain transmitter (10 dB) with three transmitters'
TII pairs 6 dB above the noise of a bin in their null symbols, tiled.  HIP-event times, the variants alternating, every
sample a window of at least 0.1 s, median of the samples with min and max for the spread:
  (a) the call (both kernels, the per-frame pair powers in the library's own buffer);
  (b) what a caller does today: vit_ofdm_fft_dev with nsyms = 1 on a start table shifted by `offset` (phase0 shifted with
      it, so the spectra are the call's), then torch: gather the 1536 bins, square, sum over repetitions and frames, the
      lower median by kthvalue, compare.  Its masks must equal the call's;
  (c) a device-to-device copy of the bytes (a) reads (nfft samples per frame);
  and, float32 only, vit_ofdm_sync_dev (75 guards) on the same frames.
Nothing is asserted about the times.  Parity: every word of the first and the last group equals the numpy model of
tests/test_tii_host.py, and the masks name the three transmitters.

usage: bench_tii.py [samples] [--out FILE]   (FILE defaults to profiles/r16_tii_bench.json)"""
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
from test_iqfmt_host import IQ_CU8, quantise  # noqa: E402
from test_ofdm_host import MODE_I  # noqa: E402
from test_sync_host import Params, prs_table, transmit_frames  # noqa: E402
from test_tii_host import Tii, add_null_symbols, expected_masks, mask_of_main_id, masks_of, tii_model  # noqa: E402

V = _vitpkg.load_package()
assert V.initialize() and V.device_count() >= 1, V.last_error()
args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "r16_tii_bench.json")
if "--out" in args:
    out_path = args[args.index("--out") + 1]
    del args[args.index("--out"):args.index("--out") + 2]
samples = int(args[0]) if args else 9
rng = np.random.default_rng(2036)
NFFT, K, NSYMS, FIC_SYMS, CIFS = MODE_I
G, NULL, SS, FS, BASE = 504, 2656, 2552, 196608, 4
W, M, NCO_BITS = 64, 16, 12
GP, C_, R, NAVG, THR = 8, 24, 4, 8, 2.5
P = Tii(NFFT, GP, C_, R, navg=NAVG, thr=THR, offset=-SS)
TXS = [(mask_of_main_id(pid), c) for pid, c in ((5, 2), (33, 11), (60, 20))]
PAD = 2 * W + 2  # behind the last frame: vit_ofdm_sync_dev's last window fits
bins = V.freq_interleave_bins(NFFT)
pairs = V.tii_pair_bins(1)
tw, nco = V.fft_twiddles(NFFT), V.nco_table(NCO_BITS)
d_tw, d_nco = torch.from_numpy(tw).cuda(), torch.from_numpy(nco).cuda()
d_pairs = torch.from_numpy(pairs.reshape(-1).view(np.int16)).cuda()
prs = prs_table(rng, NFFT, bins)
d_prs = torch.from_numpy(prs).cuda()
prm = Params(NFFT, G, NSYMS, W, M)
base, true, _ = transmit_frames(rng, prm, prs, bins, BASE, [0.0] * BASE, lead=[NULL] * BASE, tail=[0] * BASE, snr_db=10.0)
assert base.size == BASE * FS and (np.diff(true) == FS).all() and true[0] == NULL + G
base = add_null_symbols(rng, base, true, prm, P, pairs, TXS, 10.0 ** ((6.0 - 10.0) / 20.0), null_len=NULL)
raw8, SCALE8 = quantise(base, IQ_CU8)
FORMATS = {"f32": (V.IQ_F32, 1.0, 8), "cu8": (IQ_CU8, SCALE8, 2)}
STEP = 0xFFFFF000  # a small negative step: the rotation runs, the carriers stay in their bins
K_LO = torch.from_numpy(pairs.reshape(R, GP * C_).astype(np.int64)).cuda()


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


def stat(ms_t, n):
    ms, t = ms_t
    return {"ms": round(ms, 4), "ms_min_max": [round(min(t), 4), round(max(t), 4)], "us_per_frame": round(ms * 1e3 / n, 4)}


def stream_of(name, n):
    """n frame periods of the format and PAD samples of the first frame's null behind them"""
    host = base if name == "f32" else raw8
    d = torch.from_numpy(host.reshape((BASE, FS) + host.shape[1:])).cuda()
    d = d.repeat((-(-n // BASE),) + (1,) * (d.dim() - 1))[:n].reshape((n * FS,) + host.shape[1:])
    return torch.cat([d, d[:PAD]]).reshape(-1)


def today(name, d_iq, n, d_shift, d_rot_shift, d_fft, d_masks):
    fmt, scale, _ = FORMATS[name]
    V.ofdm_fft_dev(d_iq, NFFT, 1, n, d_tw, SS, d_fft, d_start=d_shift, d_nco=d_nco, nco_bits=NCO_BITS, d_rot=d_rot_shift,
                   iq_format=fmt, iq_scale=scale)
    X = torch.view_as_real(d_fft.view(n, NFFT))
    pw = (X * X).sum(dim=2)
    f = (pw[:, K_LO] + pw[:, K_LO + 1]).sum(dim=1)       # (n, Gp*C)
    E = f.view(n // NAVG, NAVG, GP * C_).sum(dim=1)
    noise = torch.kthvalue(E, (GP * C_ - 1) // 2 + 1, dim=1).values
    on = ((E > 0) & (E >= THR * noise[:, None])).view(-1, GP, C_).to(torch.int32)
    d_masks.copy_((on << torch.arange(GP, device="cuda", dtype=torch.int32)[None, :, None]).sum(dim=1))


result = {"shape": list(MODE_I), "frame_period": FS, "ngroups": GP, "ncombs": C_, "nrep": R, "navg": NAVG, "thr": THR,
          "offset": P.offset, "sizes": {}}
ok_all = True
for n in (512, 4096):
    entry = {"nframes": n}
    starts = true[0] + FS * np.arange(n, dtype=np.int64)
    rot = np.zeros((n, 2), np.uint32)
    rot[:, 0], rot[:, 1] = rng.integers(0, 1 << 32, n, dtype=np.uint64), STEP
    rot_shift = rot.copy()
    rot_shift[:, 0] = (rot[:, 0].astype(np.uint64) + (P.offset % (1 << 32)) * STEP % (1 << 32)) % (1 << 32)
    d_start, d_shift = torch.from_numpy(starts).cuda(), torch.from_numpy(starts + P.offset).cuda()
    d_rot = torch.from_numpy(rot.view(np.int32)).cuda()
    d_rot_shift = torch.from_numpy(rot_shift.view(np.int32)).cuda()
    for name, (fmt, scale, sb) in FORMATS.items():
        d_iq = stream_of(name, n)
        nbytes = n * NFFT * sb
        d_tii = torch.zeros((n // NAVG, 2 + 2 * C_), dtype=torch.int32, device="cuda")
        d_fft = torch.zeros(n * NFFT, dtype=torch.complex64, device="cuda")
        d_masks = torch.zeros((n // NAVG, C_), dtype=torch.int32, device="cuda")
        src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        fns = [lambda: V.ofdm_tii_dev(d_iq, NFFT, n, d_tw, d_pairs, d_tii, GP, C_, R, NAVG, THR, P.offset, d_start=d_start,
                                      d_nco=d_nco, nco_bits=NCO_BITS, d_rot=d_rot, iq_format=fmt, iq_scale=scale),
               lambda: today(name, d_iq, n, d_shift, d_rot_shift, d_fft, d_masks), lambda: dst.copy_(src)]
        if name == "f32":
            so = (torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros((n, 2), dtype=torch.int32, device="cuda"))
            fns.append(lambda: V.ofdm_sync_dev(d_iq, NFFT, NSYMS, n, d_tw, SS, d_nco, NCO_BITS, d_prs, so[0], so[1], W, M,
                                               frame_stride=FS, first_start=int(true[0])))
        res = alternate(fns)
        torch.cuda.synchronize()
        words = d_tii.cpu().numpy().view(np.uint32)
        host = d_iq.view(-1, 2) if name != "f32" else d_iq
        par = True  # every word of the first and the last group against the model
        for g in (0, n // NAVG - 1):
            lo = g * NAVG
            x = host[lo * FS:(lo + NAVG) * FS].cpu().numpy()
            w, _ = tii_model(x, starts[:NAVG], P, pairs, tw, nco, NCO_BITS, rot[lo:lo + NAVG], None if name == "f32" else (fmt, scale))
            par = par and np.array_equal(w[0], words[g])
        found = bool((masks_of(words) == expected_masks(P, TXS)[None, :]).all())
        differs = int((d_masks.cpu().numpy().view(np.uint32) != masks_of(words)).sum())
        e = {"read_bytes": nbytes, "tii": dict(stat(res[0], n), read_tb_per_s=round(nbytes / (res[0][0] * 1e-3) / 1e12, 4)),
             "fft_then_torch": stat(res[1], n), "copy_of_the_bytes_read": stat(res[2], n),
             "speedup_over_fft_then_torch": round(res[1][0] / res[0][0], 3), "ratio_to_copy": round(res[0][0] / res[2][0], 3),
             "masks_differing_from_fft_then_torch": differs, "transmitters_found_in_every_group": found, "parity_ok": bool(par)}
        if name == "f32":
            e["ofdm_sync_cp75"] = stat(res[3], n)
            e["ratio_to_sync"] = round(res[0][0] / res[3][0], 4)
        ok_all = ok_all and par and differs == 0
        entry[name] = e
        del d_iq, d_fft, src, dst
    result["sizes"][str(n)] = entry
text = json.dumps(result)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text + "\n")
print(text)
sys.exit(0 if ok_all else 1)
