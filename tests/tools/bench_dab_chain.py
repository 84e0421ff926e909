#!/usr/bin/env python3
"""After the decoder: what the post-passes cost.  HIP-event times (10 calls per sample, the two paths alternating, median
of the samples) of
  - 65536 FIC frames (768 bits, FIC-shaped puncturing): vit_decode_fic_dev against vit_decode_punctured_dev;
  - a config-5-sized DAB+ batch (16384 superframes, RSDims 24, punctured): vit_dabplus_punctured_superframes_dev
    against vit_decode_punctured_dev + vit_rs_batch_dev on the same input;
and a parity sample of each (distinct frames tiled: every tile equals the oracle's decode XOR the PRBS, every flag the
model's).  The post kernels' own times come from a separate `rocprofv3 --kernel-trace --stats` run of this script
(profiles/r06_dab_chain_kstats.csv).

usage: bench_dab_chain.py [samples]"""
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
from test_dab_host import fib_ok_model, fire_ok_model, scramble  # noqa: E402
from test_gpu_dab import channel, dabplus_superframes, dabplus_symbols, fic_frames  # noqa: E402
from test_punct_host import KEEP_24, KEEP_TAIL_12, depuncture, fic_segments, puncture  # noqa: E402

V = _vitpkg.load_package()
O = _vitpkg.load_oracle()
O.build()
assert V.initialize() and V.device_count() >= 1, V.last_error()
V.set_renorm_ge(0)
samples = int(sys.argv[1]) if len(sys.argv) > 1 else 15
rng = np.random.default_rng(2026)


def sample(fn, k=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / k


def alternate(fa, fb, warm=5):
    for _ in range(warm):  # code objects, scratch growth
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(samples):
        ta.append(sample(fa))
        tb.append(sample(fb))
    return float(np.median(ta)), float(np.median(tb)), ta, tb


# ---- FIC: 65536 frames, 256 distinct ones tiled ----------------------------------------------------------------------
framebits, base_n, reps = 768, 256, 256
segs = fic_segments()
_, frames = fic_frames(rng, base_n, framebits)
punct = puncture(channel(O, scramble(frames, framebits), framebits, rng, "3dB"), segs, framebits)
dec = O.decode_batch(framebits, depuncture(punct, segs, framebits, 128), nthreads=16)
want = scramble(dec, framebits)
want_ok = fib_ok_model(want.reshape(-1, 32)).reshape(base_n, 3)
n = base_n * reps
d_in = torch.from_numpy(punct).cuda().repeat(reps, 1).contiguous()
d_fibs = torch.zeros((n, 96), dtype=torch.uint8, device="cuda")
d_ok = torch.zeros((n, 3), dtype=torch.uint8, device="cuda")
d_dec = torch.zeros_like(d_fibs)
ms_fic, ms_punct, t_fic, t_punct = alternate(lambda: V.decode_fic_dev(d_in, d_fibs, d_ok, framebits, n, segs),
                                             lambda: V.decode_punctured_dev(d_in, d_dec, framebits, n, segs))
fic_parity = bool((d_fibs.view(reps, base_n, -1) == torch.from_numpy(want).cuda().unsqueeze(0)).all()) and \
    bool((d_ok.view(reps, base_n, 3) == torch.from_numpy(want_ok).cuda().unsqueeze(0)).all()) and \
    bool((d_dec.view(reps, base_n, -1) == torch.from_numpy(dec).cuda().unsqueeze(0)).all())
del d_in, d_fibs, d_ok, d_dec

# ---- DAB+: 16384 superframes x RSDims 24, 64 distinct ones tiled ------------------------------------------------------
rsdims, nsf, base_sf = 24, 16384, 64
fb = 192 * rsdims
_, sf = dabplus_superframes(rng, base_sf, rsdims)
dsegs = [(fb, KEEP_24), (6, KEEP_TAIL_12)]
dpunct = puncture(dabplus_symbols(O, rng, sf, rsdims, ["3dB"] * base_sf), dsegs, fb)
work_ref = scramble(O.decode_batch(fb, depuncture(dpunct, dsegs, fb, 128), nthreads=16), fb).reshape(base_sf, -1)
ret_ref, out_ref = O.rs_check_batch(work_ref, rsdims)
fire_ref = fire_ok_model(work_ref)
sreps = nsf // base_sf
d_in = torch.from_numpy(dpunct).cuda().repeat(sreps, 1).contiguous()
d_work = torch.zeros((nsf, 120 * rsdims), dtype=torch.uint8, device="cuda")
d_out = torch.zeros((nsf, 110 * rsdims), dtype=torch.uint8, device="cuda")
d_ret = torch.zeros(nsf, dtype=torch.int32, device="cuda")
d_fire = torch.zeros(nsf, dtype=torch.uint8, device="cuda")
d_work2, d_out2, d_ret2 = torch.zeros_like(d_work), torch.zeros_like(d_out), torch.zeros_like(d_ret)


def run_fused():
    V.dabplus_punctured_superframes_dev(d_in, dsegs, d_work, d_out, d_ret, rsdims, nsf, d_fire_ok=d_fire)


def run_plain():
    V.decode_punctured_dev(d_in, d_work2, fb, 5 * nsf, dsegs)
    V.rs_batch_dev(d_work2, d_out2, d_ret2, rsdims, nsf)


ms_dab, ms_plain, t_dab, t_plain = alternate(run_fused, run_plain, warm=3)
ok_rows = ret_ref >= 0
dab_parity = bool((d_work.view(sreps, base_sf, -1) == torch.from_numpy(work_ref).cuda().unsqueeze(0)).all()) and \
    bool((d_ret.view(sreps, base_sf) == torch.from_numpy(ret_ref).cuda().unsqueeze(0)).all()) and \
    bool((d_fire.view(sreps, base_sf) == torch.from_numpy(fire_ref).cuda().unsqueeze(0)).all()) and \
    bool((d_out.view(sreps, base_sf, -1)[:, torch.from_numpy(ok_rows).cuda()] ==
          torch.from_numpy(out_ref[ok_rows]).cuda().unsqueeze(0)).all())

print(json.dumps({
    "fic": {"nframes": n, "framebits": framebits, "transmitted_symbols": int(punct.shape[1]),
            "decode_fic_ms": round(ms_fic, 4), "decode_punctured_ms": round(ms_punct, 4),
            "ratio": round(ms_fic / ms_punct, 3), "decode_fic_ms_min_max": [round(min(t_fic), 4), round(max(t_fic), 4)],
            "decode_punctured_ms_min_max": [round(min(t_punct), 4), round(max(t_punct), 4)],
            "post_pass_bytes_moved": n * (2 * 96 + 3), "fibs_ok_in_sample": int(want_ok.sum()),
            "parity_ok": fic_parity},
    "dabplus": {"nsf": nsf, "rsdims": rsdims, "framebits": fb, "transmitted_symbols_per_frame": int(dpunct.shape[1]),
                "fused_ms": round(ms_dab, 4), "decode_punctured_plus_rs_ms": round(ms_plain, 4),
                "ratio": round(ms_dab / ms_plain, 3), "fused_ms_min_max": [round(min(t_dab), 4), round(max(t_dab), 4)],
                "decode_punctured_plus_rs_ms_min_max": [round(min(t_plain), 4), round(max(t_plain), 4)],
                "post_pass_bytes_moved": nsf * (2 * 120 * rsdims + 1), "fire_ok_in_sample": int(fire_ref.sum()),
                "rs_failed_in_sample": int((ret_ref < 0).sum()), "parity_ok": dab_parity}}))
sys.exit(0 if fic_parity and dab_parity else 1)
