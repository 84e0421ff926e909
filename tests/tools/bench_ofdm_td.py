#!/usr/bin/env python3
"""From the samples: what vit_ofdm_demod_dev costs against what a caller does today.  Mode I (nfft 2048, guard 504, null
symbol 2656: 196608 samples a frame), 512 frames and 4096 frames (6.4 GB of samples, far past the Infinity Cache).
HIP-event times, the variants of one comparison alternating, every sample a window of at least 0.1 s, median of the
samples with min and max for the spread:
  - the fused call (d_fic and ring) without rotation and with it, at nco_bits 20 (an 8 MB table: every lane's phasor is a
    cache line of its own) and at nco_bits 10 (8 KB);
  - today's composition: torch.fft.fft (rocFFT) over a strided view of the useful parts, then vit_ofdm_demap_dev; with
    rotation a tensor multiply by the frame's phasors goes in front;
  - a device-to-device copy of the bytes the fused call must move, nframes*(76*2048*8 + 75*3072), half read, half written;
  - end to end at 512 frames on decodable input (5 distinct frames from the time-domain transmitter at 14 dB with a
    frequency offset of 0.3 carrier spacings, tiled; the FIC's blocks and one DAB+ sub-channel at RSDims 24 in the CIFs):
    demod + vit_decode_fic_dev + vit_dabplus_ti_superframes_dev against the two downstream calls alone.
Parity: the fused call's bytes for the first and last frames equal the numpy model; how many bytes of the composition
differ from the fused call's is counted, not asserted (rocFFT's arithmetic is its own).  The kernel's own time and its
counters come from separate rocprofv3 runs of `bench_ofdm_td.py profile` (profiles/r09_ofdm_td_kstats.csv).

usage: bench_ofdm_td.py [samples | profile]"""
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
from test_fft_host import cfo_step, front_model, time_domain  # noqa: E402
from test_gpu_dab import dabplus_superframes  # noqa: E402
from test_ofdm_host import MODE_I, demap_model, fic_bits, random_carrier_gain, transmit  # noqa: E402
from test_punct_host import KEEP_24, KEEP_TAIL_12, fic_segments, puncture  # noqa: E402
from test_ti_host import periodic_cif  # noqa: E402

V = _vitpkg.load_package()
assert V.initialize() and V.device_count() >= 1, V.last_error()
V.set_renorm_ge(0)
profile = len(sys.argv) > 1 and sys.argv[1] == "profile"
samples = int(sys.argv[1]) if len(sys.argv) > 1 and not profile else 9
rng = np.random.default_rng(2029)
NFFT, K, NSYMS, FIC_SYMS, CIFS = MODE_I
GUARD_LEN, NULL, SS, FS = 504, 2656, 2552, 196608
FIRST = NULL + GUARD_LEN  # frame 0's first useful sample
GAIN, NCO_BITS = 254.0, 20
bins = V.freq_interleave_bins(NFFT)
d_bins = torch.from_numpy(bins.view(np.int16)).cuda()
tw, nco = V.fft_twiddles(NFFT), V.nco_table(NCO_BITS)
d_tw, d_nco = torch.from_numpy(tw).cuda(), torch.from_numpy(nco).cuda()
d_nco10 = torch.from_numpy(V.nco_table(10)).cuda()
STEP = cfo_step(0.3, NFFT)


def dev_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda()


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


def moved_bytes(n):
    return n * (NSYMS * NFFT * 8 + (NSYMS - 1) * 2 * K)


def useful_view(d_iq, n):
    """the useful parts of n frames as a strided (n, 76, 2048) view of the samples"""
    return torch.as_strided(d_iq, (n, NSYMS, NFFT), (FS, SS, 1), FIRST)


# the frame's phasors as a tensor, for today's composition with rotation: phase0 = 0 for every frame
n_idx = (np.arange(NSYMS, dtype=np.uint64)[:, None] * np.uint64(SS) + np.arange(NFFT, dtype=np.uint64)[None, :])
ph_idx = ((n_idx * np.uint64(STEP)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - NCO_BITS)
d_phasor = torch.from_numpy(np.ascontiguousarray(nco[ph_idx.astype(np.int64)]).view(np.complex64)[..., 0]).cuda()


def buffers(n):
    fic = torch.zeros((n, FIC_SYMS * 2 * K), dtype=torch.uint8, device="cuda")
    ring = torch.zeros((n * CIFS, 55296), dtype=torch.uint8, device="cuda")
    return fic, ring


def fused(d_iq, n, out, d_rot=None, bits=NCO_BITS):
    V.ofdm_demod_dev(d_iq, MODE_I, d_bins, GAIN, n, d_tw, SS, FS, d_nco=None if d_rot is None else d_nco if bits == NCO_BITS else d_nco10,
                     nco_bits=bits if d_rot is not None else 0, d_rot=d_rot, d_fic=out[0], d_ring=out[1])


def today(d_iq, n, out, rotate=False):
    x = useful_view(d_iq, n)
    if rotate:
        x = x * d_phasor
    z = torch.fft.fft(x, dim=-1)
    V.ofdm_demap_dev(z, MODE_I, d_bins, GAIN, n, d_fic=out[0], d_ring=out[1])


if profile:  # for rocprofv3: the fused call alone, a few launches
    n = 512
    d_iq = torch.view_as_complex(torch.randn((n * FS, 2), dtype=torch.float32, device="cuda"))
    d_rot = dev_u32(np.tile([0, STEP], (n, 1)))
    out = buffers(n)
    for _ in range(5):
        fused(d_iq[FIRST:], n, out)
        fused(d_iq[FIRST:], n, out, d_rot)
        today(d_iq, n, out)
    torch.cuda.synchronize()
    sys.exit(0)

O = _vitpkg.load_oracle()
O.build()
result = {"shape": list(MODE_I), "sym_stride": SS, "frame_stride": FS, "gain": GAIN, "nco_bits": NCO_BITS, "sizes": {}}
ok_all = True
for n in (512, 4096):
    d_iq = torch.view_as_complex(torch.randn((n * FS, 2), dtype=torch.float32, device="cuda"))
    d_in = d_iq[FIRST:]  # the fused call counts from frame 0's start
    d_rot = dev_u32(np.tile([0, STEP], (n, 1)))
    outs = [buffers(n) for _ in range(5)]
    moved = moved_bytes(n)
    src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    res = alternate([lambda: fused(d_in, n, outs[0]), lambda: today(d_iq, n, outs[1]),
                     lambda: fused(d_in, n, outs[2], d_rot), lambda: today(d_iq, n, outs[3], True),
                     lambda: dst.copy_(src), lambda: fused(d_in, n, outs[4], d_rot, 10)])
    differ = [int((outs[a][0] != outs[b][0]).sum()) + int((outs[a][1] != outs[b][1]).sum()) for a, b in ((0, 1), (2, 3))]
    head = min(n, 4)  # parity of the first and the last frames against the model
    par = True
    for sl in (slice(0, head), slice(n - head, n)):
        parts = useful_view(d_iq, n)[sl].cpu().numpy()
        for o, rot in ((outs[0], None), (outs[2], np.tile([0, STEP], (head, 1)))):
            want = demap_model(front_model(parts, tw, nco, NCO_BITS, rot, SS), bins, MODE_I, GAIN)
            par = par and np.array_equal(o[0][sl].cpu().numpy(), want[:, :FIC_SYMS].reshape(head, -1))
            par = par and np.array_equal(o[1][sl.start * CIFS:sl.stop * CIFS].cpu().numpy(), want[:, FIC_SYMS:].reshape(head * CIFS, -1))
    spread = max(max(t) - min(t) for _, t in res[:2])
    faster = bool(res[1][0] - res[0][0] > spread)
    result["sizes"][str(n)] = {
        "nframes": n, "moved_bytes": moved, "sample_bytes": n * FS * 8,
        "ofdm_demod": dict(stat(res[0]), tb_per_s=round(moved / (res[0][0] * 1e-3) / 1e12, 3), us_per_symbol=round(res[0][0] * 1e3 / (n * NSYMS), 4)),
        "rocfft_then_demap": stat(res[1]),
        "ofdm_demod_rotating": stat(res[2]), "multiply_rocfft_then_demap": stat(res[3]),
        "ofdm_demod_rotating_nco_bits_10": stat(res[5]),
        "copy_same_bytes": dict(stat(res[4]), tb_per_s=round(moved / (res[4][0] * 1e-3) / 1e12, 3)),
        "speedup_over_composition": round(res[1][0] / res[0][0], 3),
        "speedup_over_composition_rotating": round(res[3][0] / res[2][0], 3),
        "ratio_to_copy": round(res[0][0] / res[4][0], 3), "ratio_to_copy_rotating": round(res[2][0] / res[4][0], 3),
        "bytes_differing_from_composition": differ, "of_bytes": n * (NSYMS - 1) * 2 * K,
        "faster_than_composition_by_more_than_the_spread": faster, "spread_ms": round(spread, 4), "parity_ok": bool(par)}
    ok_all = ok_all and par and faster
    del d_iq, d_in, outs, src, dst

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
xb = time_domain(zb, GUARD_LEN, cfo=0.3)
sigma = np.sqrt(NFFT * 10.0 ** (-14.0 / 10.0) / 2.0)
xb = (xb + sigma * (rng.standard_normal(xb.shape) + 1j * rng.standard_normal(xb.shape))) / NFFT
frames = np.zeros((base_frames, FS), np.complex64)
frames[:, NULL:] = xb
start = NULL + GUARD_LEN // 2  # mid-guard
reps = (n + base_frames - 1) // base_frames
d_iq = torch.from_numpy(frames).cuda().repeat(reps, 1)[:n].reshape(-1)[start:]
rot = np.tile([0, STEP], (n, 1))
d_rot = dev_u32(rot)
parts = np.stack([[frames[t, start + l * SS:start + l * SS + NFFT] for l in range(NSYMS)] for t in range(base_frames)])
want = demap_model(front_model(parts, tw, nco, NCO_BITS, rot[:base_frames], SS), bins, MODE_I, GAIN)
d_fic, d_ring = buffers(n)
nblk, nsf = 4 * n, (n * CIFS - 15) // 5
d_fibs = torch.zeros((nblk, 96), dtype=torch.uint8, device="cuda")
d_ok = torch.zeros(nblk * 3, dtype=torch.uint8, device="cuda")
d_work = torch.zeros((nsf, 120 * rsdims), dtype=torch.uint8, device="cuda")
d_out = torch.zeros((nsf, 110 * rsdims), dtype=torch.uint8, device="cuda")
d_ret = torch.zeros(nsf, dtype=torch.int32, device="cuda")
d_fire = torch.zeros(nsf, dtype=torch.uint8, device="cuda")
fsegs = fic_segments()
# the last frame's window ends before the tiled buffer does: every frame is inside nsamples


def demod():
    fused(d_iq, n, (d_fic, d_ring), d_rot)


def downstream():
    V.decode_fic_dev(d_fic, d_fibs, d_ok, 768, nblk, fsegs)
    V.dabplus_ti_superframes_dev(d_ring, 0, 0, dsegs, d_work, d_out, d_ret, rsdims, nsf, d_fire_ok=d_fire)


def chain():
    demod()
    downstream()


demod()
e2e = alternate([chain, downstream])
d_want = torch.from_numpy(np.tile(want, (reps, 1, 1))[:n]).cuda()
e2e_par = bool((d_fic.view(n, FIC_SYMS, -1) == d_want[:, :FIC_SYMS]).all()) and \
    bool((d_ring.view(n, NSYMS - 1 - FIC_SYMS, -1) == d_want[:, FIC_SYMS:]).all())
decoded_ok = bool((d_ok == 1).all()) and bool((d_fire == 1).all()) and bool((d_ret >= 0).all()) and \
    np.array_equal(d_fibs.cpu().numpy()[:4 * base_frames], fibs) and np.array_equal(d_out.cpu().numpy()[:base_sf], pay)
result["end_to_end_512"] = {"nframes": n, "fic_blocks": nblk, "dabplus_superframes": nsf, "rsdims": rsdims,
                            "chain": stat(e2e[0]), "downstream_alone": stat(e2e[1]),
                            "demod_adds_ms": round(e2e[0][0] - e2e[1][0], 4),
                            "ratio_chain_to_downstream": round(e2e[0][0] / e2e[1][0], 3),
                            "parity_ok": e2e_par, "all_crc_and_fire_codes_hold": decoded_ok}
ok_all = ok_all and e2e_par and decoded_ok
print(json.dumps(result))
sys.exit(0 if ok_all else 1)
