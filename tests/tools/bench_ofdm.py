#!/usr/bin/env python3
"""From the FFT: what vit_ofdm_demap_dev costs.  Mode I, 512 frames (2048 CIFs, the ring size bench_ti.py uses) and 4096
frames (5 GB of FFT output, far past the Infinity Cache).  HIP-event times, the variants of one comparison alternating,
every sample a window of at least 0.1 s, median of the samples with min and max for the spread:
  - the call (d_fic and ring), as time and as algorithmic bytes per second - active bins only,
    nframes*(nsyms*K*8 + (nsyms-1)*2K) - over the call's time;
  - the same result from torch ops on the device (index by bins, multiply by the conjugate of the previous row,
    normalise, quantise, split), with the number of bytes that differ from the call's (torch's complex product may round
    differently; counted, not asserted);
  - a device-to-device copy that moves the same number of bytes (half read, half written);
  - end to end at 512 frames on decodable input (5 distinct frames through the model transmitter at 14 dB, tiled; the FIC's
    blocks and one DAB+ sub-channel at RSDims 24 in the CIFs): demap + vit_decode_fic_dev + vit_dabplus_ti_superframes_dev
    against the two downstream calls alone on the buffers the demapper filled.
Parity: the call's bytes for the distinct frames equal the numpy model, every FIB CRC and fire code holds.  The kernel's
own time comes from a separate `rocprofv3 --kernel-trace --stats` run of this script (profiles/r08_ofdm_kstats.csv).

usage: bench_ofdm.py [samples]"""
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
from test_dab_host import scramble  # noqa: E402
from test_gpu_dab import dabplus_superframes  # noqa: E402
from test_ofdm_host import MODE_I, demap_model, fic_bits, random_carrier_gain, transmit  # noqa: E402
from test_punct_host import KEEP_24, KEEP_TAIL_12, fic_segments, puncture  # noqa: E402
from test_ti_host import periodic_cif  # noqa: E402

V = _vitpkg.load_package()
O = _vitpkg.load_oracle()
O.build()
assert V.initialize() and V.device_count() >= 1, V.last_error()
V.set_renorm_ge(0)
samples = int(sys.argv[1]) if len(sys.argv) > 1 else 9
rng = np.random.default_rng(2028)
NFFT, K, NSYMS, FIC_SYMS, CIFS = MODE_I
GAIN = 254.0
bins = V.freq_interleave_bins(NFFT)
d_bins = torch.from_numpy(bins.view(np.int16)).cuda()
d_idx = torch.from_numpy(bins.astype(np.int64)).cuda()


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


def torch_demap(d_fft, n, d_fic, d_ring):
    """what a user does today: tensor ops"""
    z = torch.view_as_complex(d_fft.view(n, NSYMS, NFFT, 2))[:, :, d_idx]
    y = z[:, 1:] * z[:, :-1].conj()
    re, im = y.real, y.imag
    nrm = re.abs() + im.abs()
    ok = (nrm >= 2.0 ** -64) & (nrm <= torch.finfo(torch.float32).max)
    s = GAIN / nrm
    q = torch.cat([(128 - torch.round(re * s)).clamp(0, 255), (128 - torch.round(im * s)).clamp(0, 255)], dim=2)
    out = torch.where(torch.cat([ok, ok], dim=2), q, 128.0).to(torch.uint8)
    d_fic.copy_(out[:, :FIC_SYMS].reshape(n, -1))
    d_ring.copy_(out[:, FIC_SYMS:].reshape(n * CIFS, -1))


def algorithmic_bytes(n):
    return n * (NSYMS * K * 8 + (NSYMS - 1) * 2 * K)


result = {"shape": list(MODE_I), "gain": GAIN, "sizes": {}}
ok_all = True
for n in (512, 4096):
    d_fft = torch.randn((n, NSYMS * NFFT * 2), dtype=torch.float32, device="cuda")
    fic = [torch.zeros((n, FIC_SYMS * 2 * K), dtype=torch.uint8, device="cuda") for _ in range(2)]
    ring = [torch.zeros((n * CIFS, 55296), dtype=torch.uint8, device="cuda") for _ in range(2)]
    moved = algorithmic_bytes(n)
    src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    res = alternate([lambda: V.ofdm_demap_dev(d_fft, MODE_I, d_bins, GAIN, n, d_fic=fic[0], d_ring=ring[0]),
                     lambda: torch_demap(d_fft, n, fic[1], ring[1]),
                     lambda: dst.copy_(src)])
    differ = int((fic[0] != fic[1]).sum()) + int((ring[0] != ring[1]).sum())
    off_by_more = int(((fic[0].int() - fic[1].int()).abs() > 1).sum()) + int(((ring[0].int() - ring[1].int()).abs() > 1).sum())
    head = min(n, 8)  # parity of the first and the last frames against the model
    z = d_fft.view(n, NSYMS, NFFT, 2)
    par = True
    for sl in (slice(0, head), slice(n - head, n)):
        want = demap_model(z[sl].cpu().numpy().view(np.complex64)[..., 0], bins, MODE_I, GAIN)
        par = par and np.array_equal(fic[0][sl].cpu().numpy(), want[:, :FIC_SYMS].reshape(head, -1))
        par = par and np.array_equal(ring[0][sl.start * CIFS:sl.stop * CIFS].cpu().numpy(), want[:, FIC_SYMS:].reshape(head * CIFS, -1))
    ok_all = ok_all and par
    result["sizes"][str(n)] = {
        "nframes": n, "algorithmic_bytes": moved, "fft_bytes": n * NSYMS * NFFT * 8,
        "ofdm_demap": dict(stat(res[0]), tb_per_s=round(moved / (res[0][0] * 1e-3) / 1e12, 3)),
        "torch_ops": stat(res[1]), "copy_same_bytes": dict(stat(res[2]), tb_per_s=round(moved / (res[2][0] * 1e-3) / 1e12, 3)),
        "speedup_over_torch_ops": round(res[1][0] / res[0][0], 2),
        "ratio_to_copy": round(res[0][0] / res[2][0], 3),
        "bytes_differing_from_torch_ops": differ, "of_bytes": n * (NSYMS - 1) * 2 * K, "differing_by_more_than_1": off_by_more,
        "faster_than_torch_ops": bool(res[0][0] < res[1][0]), "parity_ok": bool(par)}
    ok_all = ok_all and res[0][0] < res[1][0]
    del d_fft, fic, ring, src, dst

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
zb = transmit(bits, bins, MODE_I, rng, carrier_gain=random_carrier_gain(rng, NFFT), snr_db=14.0)
want = demap_model(zb, bins, MODE_I, GAIN)
reps = (n + base_frames - 1) // base_frames
d_fft = torch.from_numpy(zb.view(np.float32).reshape(base_frames, -1)).cuda().repeat(reps, 1)[:n].contiguous()
d_fic = torch.zeros((n, FIC_SYMS * 2 * K), dtype=torch.uint8, device="cuda")
d_ring = torch.zeros((n * CIFS, 55296), dtype=torch.uint8, device="cuda")
nblk, nsf = 4 * n, (n * CIFS - 15) // 5
d_fibs = torch.zeros((nblk, 96), dtype=torch.uint8, device="cuda")
d_ok = torch.zeros(nblk * 3, dtype=torch.uint8, device="cuda")
d_work = torch.zeros((nsf, 120 * rsdims), dtype=torch.uint8, device="cuda")
d_out = torch.zeros((nsf, 110 * rsdims), dtype=torch.uint8, device="cuda")
d_ret = torch.zeros(nsf, dtype=torch.int32, device="cuda")
d_fire = torch.zeros(nsf, dtype=torch.uint8, device="cuda")
fsegs = fic_segments()


def demap():
    V.ofdm_demap_dev(d_fft, MODE_I, d_bins, GAIN, n, d_fic=d_fic, d_ring=d_ring)


def downstream():
    V.decode_fic_dev(d_fic, d_fibs, d_ok, 768, nblk, fsegs)
    V.dabplus_ti_superframes_dev(d_ring, 0, 0, dsegs, d_work, d_out, d_ret, rsdims, nsf, d_fire_ok=d_fire)


def chain():
    demap()
    downstream()


demap()
e2e = alternate([chain, downstream])
d_want = torch.from_numpy(np.tile(want, (reps, 1, 1))[:n]).cuda()
e2e_par = bool((d_fic.view(n, FIC_SYMS, -1) == d_want[:, :FIC_SYMS]).all()) and \
    bool((d_ring.view(n, NSYMS - 1 - FIC_SYMS, -1) == d_want[:, FIC_SYMS:]).all())
decoded_ok = bool((d_ok == 1).all()) and bool((d_fire == 1).all()) and bool((d_ret >= 0).all()) and \
    np.array_equal(d_fibs.cpu().numpy()[:4 * base_frames], fibs) and np.array_equal(d_out.cpu().numpy()[:base_sf], pay)
result["end_to_end_512"] = {"nframes": n, "fic_blocks": nblk, "dabplus_superframes": nsf, "rsdims": rsdims,
                            "chain": stat(e2e[0]), "downstream_alone": stat(e2e[1]),
                            "demap_adds_ms": round(e2e[0][0] - e2e[1][0], 4),
                            "ratio_chain_to_downstream": round(e2e[0][0] / e2e[1][0], 3),
                            "parity_ok": e2e_par, "all_crc_and_fire_codes_hold": decoded_ok}
ok_all = ok_all and e2e_par and decoded_ok
print(json.dumps(result))
sys.exit(0 if ok_all else 1)
