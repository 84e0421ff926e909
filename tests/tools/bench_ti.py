#!/usr/bin/env python3
"""MSC time de-interleaving: what the standalone pass and the fused expansion cost.  HIP-event times (10 calls per sample,
the variants of one comparison alternating, median of the samples, min and max for the spread) of
  - the standalone vit_time_deinterleave_dev: 65536 frames x 2304 columns, and a 55296-column ring (one mode-I CIF)
    of 2048 + 15 rows;
  - 65536 FIC-shaped frames (768 bits, 2304 transmitted symbols): vit_decode_punctured_ti_dev from the ring, against
    vit_decode_punctured_dev on the same frames already de-interleaved, and against the two-call composition
    (vit_time_deinterleave_dev, then vit_decode_punctured_dev);
  - 16384 DAB+ superframes at RSDims 24: vit_dabplus_ti_superframes_dev from the ring against
    vit_dabplus_punctured_superframes_dev on the de-interleaved input;
with parity of every output (distinct frames repeated periodically, so the ring is periodic too: every tile equals the
oracle's decode, the standalone outputs equal the numpy model).  The kernels' own times come from a separate
`rocprofv3 --kernel-trace --stats` run of this script (profiles/r07_ti_kstats.csv).

usage: bench_ti.py [samples]"""
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
from test_dab_host import fire_ok_model, scramble  # noqa: E402
from test_gpu_dab import dabplus_superframes, dabplus_symbols  # noqa: E402
from test_punct_host import KEEP_24, KEEP_TAIL_12, depuncture, fic_segments, puncture  # noqa: E402
from test_ti_host import deinterleave, periodic_cif  # noqa: E402

V = _vitpkg.load_package()
O = _vitpkg.load_oracle()
O.build()
assert V.initialize() and V.device_count() >= 1, V.last_error()
V.set_renorm_ge(0)
samples = int(sys.argv[1]) if len(sys.argv) > 1 else 15
rng = np.random.default_rng(2027)


def sample(fn, k=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / k


def alternate(fns, warm=5):
    """median ms of each fn and its samples, the fns alternating"""
    for _ in range(warm):  # code objects, scratch growth
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(samples):
        for t, fn in zip(ts, fns):
            t.append(sample(fn))
    return [(float(np.median(t)), t) for t in ts]


def stat(ms_t):
    ms, t = ms_t
    return {"ms": round(ms, 4), "ms_min_max": [round(min(t), 4), round(max(t), 4)]}


def periodic_ring(base, nrows):
    """periodic_cif(base, nrows) built on the device from one period of rows: frame n = base[n % len(base)]"""
    nb = base.shape[0]
    period = periodic_cif(base, nb)
    return torch.from_numpy(period).cuda().repeat((nrows + nb - 1) // nb, 1)[:nrows].contiguous()


# ---- standalone -----------------------------------------------------------------------------------------------------
standalone = {}
for name, nframes, ncols in (("fic_width", 65536, 2304), ("mode1_cif", 2048, 55296)):
    d_ring = torch.randint(0, 256, (nframes + 15, ncols), dtype=torch.uint8, device="cuda")
    d_out = torch.zeros((nframes, ncols), dtype=torch.uint8, device="cuda")
    (res,) = alternate([lambda: V.time_deinterleave_dev(d_ring, 0, 0, ncols, d_out, nframes)])
    head = min(nframes, 64)  # parity: the first and the last frames against the model
    ok = np.array_equal(d_out[:head].cpu().numpy(), deinterleave(d_ring[:head + 15].cpu().numpy(), 0, 0, ncols, head))
    tail = d_ring[nframes - head:].cpu().numpy()
    ok = ok and np.array_equal(d_out[nframes - head:].cpu().numpy(), deinterleave(tail, 0, 0, ncols, head))
    moved = (2 * nframes + 15) * ncols
    standalone[name] = dict(nframes=nframes, ncols=ncols, bytes_moved=moved, **stat(res),
                            tb_per_s=round(moved / (res[0] * 1e-3) / 1e12, 3), parity_ok=bool(ok))
    del d_ring, d_out

# ---- fused: 65536 FIC frames, 256 distinct ones ------------------------------------------------------------------------
framebits, base_n, n = 768, 256, 65536
segs = fic_segments()
a = O.noisy_frames(base_n // 2, framebits, seed=5)
b = O.uniform_symbols((base_n // 2) * O.sym_len(framebits), seed=6).reshape(base_n // 2, -1)
punct = puncture(np.concatenate([a, b]), segs, framebits)
P = punct.shape[1]
want = torch.from_numpy(O.decode_batch(framebits, depuncture(punct, segs, framebits, 128), nthreads=16)).cuda()
d_ring = periodic_ring(punct, n + 15)
d_deint = torch.from_numpy(punct).cuda().repeat(n // base_n, 1).contiguous()
d_tmp = torch.zeros_like(d_deint)
outs = [torch.zeros((n, framebits // 8), dtype=torch.uint8, device="cuda") for _ in range(3)]


def composition():
    V.time_deinterleave_dev(d_ring, 0, 0, P, d_tmp, n)
    V.decode_punctured_dev(d_tmp, outs[2], framebits, n, segs)


fused = alternate([lambda: V.decode_punctured_ti_dev(d_ring, 0, 0, outs[0], framebits, n, segs),
                   lambda: V.decode_punctured_dev(d_deint, outs[1], framebits, n, segs),
                   composition])
fused_parity = all(bool((o.view(n // base_n, base_n, -1) == want.unsqueeze(0)).all()) for o in outs) and \
    bool((d_tmp == d_deint).all())
fic = {"nframes": n, "framebits": framebits, "transmitted_symbols": P,
       "decode_punctured_ti": stat(fused[0]), "decode_punctured_deinterleaved": stat(fused[1]),
       "composition": stat(fused[2]),
       "ratio_ti_to_punctured": round(fused[0][0] / fused[1][0], 3),
       "ratio_composition_to_punctured": round(fused[2][0] / fused[1][0], 3), "parity_ok": fused_parity}
del d_ring, d_deint, d_tmp, outs

# ---- DAB+: 16384 superframes x RSDims 24, 64 distinct ones ------------------------------------------------------------
rsdims, nsf, base_sf = 24, 16384, 64
fb = 192 * rsdims
_, sf = dabplus_superframes(rng, base_sf, rsdims)
dsegs = [(fb, KEEP_24), (6, KEEP_TAIL_12)]
dpunct = puncture(dabplus_symbols(O, rng, sf, rsdims, ["3dB"] * base_sf), dsegs, fb)
work_ref = scramble(O.decode_batch(fb, depuncture(dpunct, dsegs, fb, 128), nthreads=16), fb).reshape(base_sf, -1)
sreps = nsf // base_sf
d_ring = periodic_ring(dpunct, 5 * nsf + 15)
d_in = torch.from_numpy(dpunct).cuda().repeat(sreps, 1).contiguous()
bufs = [(torch.zeros((nsf, 120 * rsdims), dtype=torch.uint8, device="cuda"),
         torch.zeros((nsf, 110 * rsdims), dtype=torch.uint8, device="cuda"),
         torch.zeros(nsf, dtype=torch.int32, device="cuda"), torch.zeros(nsf, dtype=torch.uint8, device="cuda"))
        for _ in range(2)]
dab = alternate([lambda: V.dabplus_ti_superframes_dev(d_ring, 0, 0, dsegs, *bufs[0][:3], rsdims, nsf, d_fire_ok=bufs[0][3]),
                 lambda: V.dabplus_punctured_superframes_dev(d_in, dsegs, *bufs[1][:3], rsdims, nsf, d_fire_ok=bufs[1][3])],
                warm=3)
dab_parity = all(bool((x == y).all()) for x, y in zip(*bufs)) and \
    bool((bufs[0][0].view(sreps, base_sf, -1) == torch.from_numpy(work_ref).cuda().unsqueeze(0)).all()) and \
    bool((bufs[0][3].view(sreps, base_sf) == torch.from_numpy(fire_ok_model(work_ref)).cuda().unsqueeze(0)).all())
dabplus = {"nsf": nsf, "rsdims": rsdims, "framebits": fb, "transmitted_symbols_per_frame": int(dpunct.shape[1]),
           "dabplus_ti": stat(dab[0]), "dabplus_punctured_deinterleaved": stat(dab[1]),
           "ratio": round(dab[0][0] / dab[1][0], 3), "parity_ok": dab_parity}

print(json.dumps({"standalone": standalone, "fused_fic": fic, "dabplus": dabplus}))
ok = all(v["parity_ok"] for v in standalone.values()) and fused_parity and dab_parity
sys.exit(0 if ok else 1)
