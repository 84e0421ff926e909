#!/usr/bin/env python3
"""Channel-state weighting: what the per-symbol soft-decision rule costs against the existing calls on the same buffers.
Mode I (nfft 2048, guard 504, null symbol 2656: 196608 samples a frame), 512 frames and 4096 frames.  HIP-event times,
the variants of one comparison alternating, every sample a window of at least 0.1 s, median of the samples with min and
max for the spread:
  - vit_ofdm_demod_dev (gain 254) against vit_ofdm_demod_soft_dev (VIT_SOFT_PER_SYMBOL, gain 64, with d_level) on float32
    samples, and vit_ofdm_demod_iq_dev against vit_ofdm_demod_soft_dev on the same samples as cu8;
  - vit_ofdm_demap_dev against vit_ofdm_demap_soft_dev on the spectra vit_ofdm_fft_dev makes of the float32 samples;
  - a device-to-device copy of the bytes the demapper must move - the active bins in, the soft bytes out:
    nframes*(76*1536*8 + 75*3072), half read, half written;
  - end to end at 512 frames on decodable input (5 distinct frames from the time-domain transmitter at 14 dB, tiled; the
    FIC's blocks and one DAB+ sub-channel at RSDims 24 in the CIFs): either demodulator + vit_decode_fic_dev +
    vit_dabplus_ti_superframes_dev, and the two downstream calls alone.
No cost ratio is asserted (none was fixed in advance): the ratios and the spread are reported.  Parity is: the per-symbol
calls' bytes and levels for the first and last frames equal the numpy model of tests/test_csi_host.py, the two per-symbol
calls agree in every byte and level word, and the chain behind the per-symbol rule decodes what was sent.

usage: bench_csi.py [samples]"""
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
from test_csi_host import demap_soft_model  # noqa: E402
from test_dab_host import scramble  # noqa: E402
from test_fft_host import front_model, time_domain  # noqa: E402
from test_gpu_dab import dabplus_superframes  # noqa: E402
from test_iqfmt_host import IQ_CU8, convert_model  # noqa: E402
from test_ofdm_host import MODE_I, fic_bits, random_carrier_gain, transmit  # noqa: E402
from test_punct_host import KEEP_24, KEEP_TAIL_12, fic_segments, puncture  # noqa: E402
from test_ti_host import periodic_cif  # noqa: E402

V = _vitpkg.load_package()
assert V.initialize() and V.device_count() >= 1, V.last_error()
V.set_renorm_ge(0)
samples = int(sys.argv[1]) if len(sys.argv) > 1 else 9
rng = np.random.default_rng(2031)
NFFT, K, NSYMS, FIC_SYMS, CIFS = MODE_I
GUARD_LEN, NULL, SS, FS = 504, 2656, 2552, 196608
FIRST = NULL + GUARD_LEN  # frame 0's first useful sample
GAIN_CARRIER, GAIN_SYMBOL, CU8_SCALE = 254.0, 64.0, 2.0 ** -8
bins = V.freq_interleave_bins(NFFT)
d_bins = torch.from_numpy(bins.view(np.int16)).cuda()
tw = V.fft_twiddles(NFFT)
d_tw = torch.from_numpy(tw).cuda()


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


def compare(old, new):
    """the per-symbol call against the existing one: ratio of the medians, the larger spread of the two, and whether the
    difference exceeds it"""
    spread = max(max(t) - min(t) for _, t in (old, new))
    return {"existing": stat(old), "per_symbol": stat(new), "ratio": round(new[0] / old[0], 3), "spread_ms": round(spread, 4),
            "slower_by_more_than_the_spread": bool(new[0] - old[0] > spread)}


def buffers(n, level=False):
    fic = torch.zeros((n, FIC_SYMS * 2 * K), dtype=torch.uint8, device="cuda")
    ring = torch.zeros((n * CIFS, 55296), dtype=torch.uint8, device="cuda")
    return (fic, ring, torch.zeros((n, NSYMS - 1), dtype=torch.float32, device="cuda")) if level else (fic, ring)


def demod(d_iq, n, out, iq_format=V.IQ_F32):
    V.ofdm_demod_dev(d_iq, MODE_I, d_bins, GAIN_CARRIER, n, d_tw, SS, FS, d_fic=out[0], d_ring=out[1], iq_format=iq_format,
                     iq_scale=CU8_SCALE)


def demod_soft(d_iq, n, out, iq_format=V.IQ_F32):
    V.ofdm_demod_soft_dev(d_iq, MODE_I, d_bins, V.SOFT_PER_SYMBOL, GAIN_SYMBOL, n, d_tw, SS, FS, d_fic=out[0], d_ring=out[1],
                          d_level=out[2], iq_format=iq_format, iq_scale=CU8_SCALE)


def demap(d_fft, n, out):
    V.ofdm_demap_dev(d_fft, MODE_I, d_bins, GAIN_CARRIER, n, d_fic=out[0], d_ring=out[1])


def demap_soft(d_fft, n, out):
    V.ofdm_demap_soft_dev(d_fft, MODE_I, d_bins, V.SOFT_PER_SYMBOL, GAIN_SYMBOL, n, d_fic=out[0], d_ring=out[1], d_level=out[2])


def equals_model(out, parts, sl, head):
    """a per-symbol call's bytes and levels of the frames sl against the model on their useful parts"""
    want, S = demap_soft_model(front_model(parts, tw), bins, MODE_I, GAIN_SYMBOL)
    return (np.array_equal(out[0][sl].cpu().numpy(), want[:, :FIC_SYMS].reshape(head, -1))
            and np.array_equal(out[1][sl.start * CIFS:sl.stop * CIFS].cpu().numpy(), want[:, FIC_SYMS:].reshape(head * CIFS, -1))
            and np.array_equal(out[2][sl].cpu().numpy().view(np.uint32), S.view(np.uint32)))


O = _vitpkg.load_oracle()
O.build()
result = {"shape": list(MODE_I), "sym_stride": SS, "frame_stride": FS, "gain_per_carrier": GAIN_CARRIER,
          "gain_per_symbol": GAIN_SYMBOL, "samples": samples, "sizes": {}}
ok_all = True
for n in (512, 4096):
    d_raw = torch.randint(0, 256, (n * FS, 2), dtype=torch.uint8, device="cuda")
    d_iq = torch.empty(n * FS, dtype=torch.complex64, device="cuda")
    V.iq_convert_dev(d_raw.view(-1), IQ_CU8, CU8_SCALE, d_iq)  # the same samples in both formats
    d_in, d_in8 = d_iq[FIRST:], d_raw[FIRST:].reshape(-1)  # the calls count from frame 0's start
    d_fft = torch.empty((n, NSYMS, NFFT), dtype=torch.complex64, device="cuda")
    V.ofdm_fft_dev(d_in, NFFT, NSYMS, n, d_tw, SS, d_fft, frame_stride=FS)
    old = [buffers(n) for _ in range(3)]
    new = [buffers(n, True) for _ in range(3)]
    moved = n * (NSYMS * K * 8 + (NSYMS - 1) * 2 * K)  # the demapper never loads a bin no carrier uses
    src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    res = alternate([lambda: demod(d_in, n, old[0]), lambda: demod_soft(d_in, n, new[0]),
                     lambda: demod(d_in8, n, old[1], IQ_CU8), lambda: demod_soft(d_in8, n, new[1], IQ_CU8),
                     lambda: demap(d_fft, n, old[2]), lambda: demap_soft(d_fft, n, new[2]),
                     lambda: dst.copy_(src)])
    # parity: the three per-symbol calls agree in every byte and level word; the first and last frames equal the model
    par = all(torch.equal(a, b) for o in new[1:] for a, b in zip(new[0], o))
    same_as_before = all(torch.equal(a, b) for o in old[1:] for a, b in zip(old[0], o))
    head = min(n, 2)
    for sl in (slice(0, head), slice(n - head, n)):
        raw = torch.as_strided(d_raw, (n, NSYMS, NFFT, 2), (FS * 2, SS * 2, 2, 1), FIRST * 2)[sl].cpu().numpy()
        par = par and equals_model(new[1], convert_model(raw, IQ_CU8, CU8_SCALE), sl, head)
    result["sizes"][str(n)] = {
        "nframes": n, "moved_bytes": moved,
        "ofdm_demod_float32": compare(res[0], res[1]), "ofdm_demod_cu8": compare(res[2], res[3]),
        "ofdm_demap": compare(res[4], res[5]),
        "copy_same_bytes": dict(stat(res[6]), tb_per_s=round(moved / (res[6][0] * 1e-3) / 1e12, 3)),
        "ofdm_demap_ratio_to_copy": {"existing": round(res[4][0] / res[6][0], 3), "per_symbol": round(res[5][0] / res[6][0], 3)},
        "parity_ok": bool(par), "existing_calls_agree": bool(same_as_before)}
    ok_all = ok_all and par and same_as_before
    del d_raw, d_iq, d_in, d_in8, d_fft, old, new, src, dst

# ---- end to end at 512 frames: decodable input --------------------------------------------------------------------------
n, base_frames, rsdims = 512, 5, 24
fb = 192 * rsdims
fibs, fic_tx = fic_bits(O, rng, base_frames)
base_sf = 5 * base_frames * CIFS // 25  # 20 logical frames a period: 4 superframes
pay, sf = dabplus_superframes(rng, base_sf, rsdims)
coded = np.stack([O.encode(b) for b in np.unpackbits(scramble(sf.reshape(-1, 24 * rsdims), fb), axis=1)]).astype(np.uint8)
dsegs = [(fb, KEEP_24), (6, KEEP_TAIL_12)]
punct = puncture(coded, dsegs, fb)
P = punct.shape[1]
cif = rng.integers(0, 2, (base_frames * CIFS, 55296), dtype=np.uint8)
cif[:, :P] = periodic_cif(punct, base_frames * CIFS)
bits = np.zeros((base_frames, NSYMS - 1, 2 * K), np.int64)
bits[:, :FIC_SYMS] = fic_tx
bits[:, FIC_SYMS:] = cif.reshape(base_frames, NSYMS - 1 - FIC_SYMS, 2 * K)
zb = transmit(bits, bins, MODE_I, rng, carrier_gain=random_carrier_gain(rng, NFFT))
xb = time_domain(zb, GUARD_LEN)
sigma = np.sqrt(NFFT * 10.0 ** (-14.0 / 10.0) / 2.0)
xb = (xb + sigma * (rng.standard_normal(xb.shape) + 1j * rng.standard_normal(xb.shape))) / NFFT
frames = np.zeros((base_frames, FS), np.complex64)
frames[:, NULL:] = xb
start = NULL + GUARD_LEN // 2  # mid-guard
reps = (n + base_frames - 1) // base_frames
d_iq = torch.from_numpy(frames).cuda().repeat(reps, 1)[:n].reshape(-1)[start:]
parts = np.stack([[frames[t, start + l * SS:start + l * SS + NFFT] for l in range(NSYMS)] for t in range(base_frames)])
want, want_S = demap_soft_model(front_model(parts, tw), bins, MODE_I, GAIN_SYMBOL)
out_old, out_new = buffers(n), buffers(n, True)
nblk, nsf = 4 * n, (n * CIFS - 15) // 5
d_fibs = torch.zeros((nblk, 96), dtype=torch.uint8, device="cuda")
d_ok = torch.zeros(nblk * 3, dtype=torch.uint8, device="cuda")
d_work = torch.zeros((nsf, 120 * rsdims), dtype=torch.uint8, device="cuda")
d_out = torch.zeros((nsf, 110 * rsdims), dtype=torch.uint8, device="cuda")
d_ret = torch.zeros(nsf, dtype=torch.int32, device="cuda")
d_fire = torch.zeros(nsf, dtype=torch.uint8, device="cuda")
fsegs = fic_segments()


def downstream(out):
    V.decode_fic_dev(out[0], d_fibs, d_ok, 768, nblk, fsegs)
    V.dabplus_ti_superframes_dev(out[1], 0, 0, dsegs, d_work, d_out, d_ret, rsdims, nsf, d_fire_ok=d_fire)


def chain_old():
    demod(d_iq, n, out_old)
    downstream(out_old)


def chain_new():
    demod_soft(d_iq, n, out_new)
    downstream(out_new)


demod_soft(d_iq, n, out_new)
e2e = alternate([chain_old, chain_new, lambda: downstream(out_new)])
chain_new()  # the decoded outputs below are the per-symbol chain's
torch.cuda.synchronize()
d_want = torch.from_numpy(np.tile(want, (reps, 1, 1))[:n]).cuda()
e2e_par = bool((out_new[0].view(n, FIC_SYMS, -1) == d_want[:, :FIC_SYMS]).all()) and \
    bool((out_new[1].view(n, NSYMS - 1 - FIC_SYMS, -1) == d_want[:, FIC_SYMS:]).all()) and \
    np.array_equal(out_new[2].cpu().numpy().view(np.uint32), np.tile(want_S, (reps, 1))[:n].view(np.uint32))
decoded_ok = bool((d_ok == 1).all()) and bool((d_fire == 1).all()) and bool((d_ret >= 0).all()) and \
    np.array_equal(d_fibs.cpu().numpy()[:4 * base_frames], fibs) and np.array_equal(d_out.cpu().numpy()[:base_sf], pay)
result["end_to_end_512"] = dict(compare(e2e[0], e2e[1]), nframes=n, fic_blocks=nblk, dabplus_superframes=nsf, rsdims=rsdims,
                                downstream_alone=stat(e2e[2]), parity_ok=e2e_par, all_crc_and_fire_codes_hold=decoded_ok)
ok_all = ok_all and e2e_par and decoded_ok
print(json.dumps(result))
sys.exit(0 if ok_all else 1)
