#!/usr/bin/env python3
"""Punctured input: 65536 FIC-shaped frames (768 bits, 2304 transmitted symbols) through vit_decode_punctured_dev
against the same frames, depunctured, through vit_decode_batch_dev.  HIP-event times (10 calls per sample, the two
paths alternating, median of the samples), the bytes the expansion pass moves, and a parity sample (256 distinct
frames tiled: every tile of both outputs equals the oracle's decode).  The expansion kernel's own time comes from a
separate `rocprofv3 --kernel-trace --stats` run of this script (profiles/r05_punct_kstats.csv).

usage: bench_punctured.py [nframes] [samples]"""
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
from test_punct_host import depuncture, fic_segments, puncture  # noqa: E402

V = _vitpkg.load_package()
O = _vitpkg.load_oracle()
O.build()
assert V.initialize() and V.device_count() >= 1, V.last_error()
V.set_renorm_ge(0)
nframes = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
samples = int(sys.argv[2]) if len(sys.argv) > 2 else 15
framebits, base_n, erasure = 768, 256, 128
segs = fic_segments()
P = V.punctured_length(segs, framebits)
T = framebits + 6
reps = nframes // base_n
nframes = reps * base_n

a = O.noisy_frames(base_n // 2, framebits, seed=5)
b = O.uniform_symbols((base_n // 2) * O.sym_len(framebits), seed=6).reshape(base_n // 2, -1)
punct = puncture(np.concatenate([a, b]), segs, framebits)
full = depuncture(punct, segs, framebits, erasure)
want = O.decode_batch(framebits, full, nthreads=8)

d_punct = torch.from_numpy(punct).cuda().repeat(reps, 1).contiguous()
d_full = torch.from_numpy(full).cuda().repeat(reps, 1).contiguous()
d_out_p = torch.zeros((nframes, framebits // 8), dtype=torch.uint8, device="cuda")
d_out_u = torch.zeros_like(d_out_p)


def run_p():
    V.decode_punctured_dev(d_punct, d_out_p, framebits, nframes, segs, erasure)


def run_u():
    V.decode_batch_dev(d_full, d_out_u, framebits, nframes)


for _ in range(5):  # warm-up: code objects, scratch growth
    run_p()
    run_u()
torch.cuda.synchronize()


def sample(fn, k=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / k


tp, tu = [], []
for _ in range(samples):
    tp.append(sample(run_p))
    tu.append(sample(run_u))
ms_p, ms_u = float(np.median(tp)), float(np.median(tu))
d_want = torch.from_numpy(want).cuda().unsqueeze(0)
parity = bool((d_out_p.view(reps, base_n, -1) == d_want).all()) and bool((d_out_u.view(reps, base_n, -1) == d_want).all())
moved = nframes * (P + 4 * T)
print(json.dumps({
    "nframes": nframes, "framebits": framebits, "transmitted_symbols": P, "depunctured_symbols": 4 * T,
    "punctured_ms": round(ms_p, 4), "unpunctured_ms": round(ms_u, 4), "ratio": round(ms_p / ms_u, 3),
    "punctured_ms_min_max": [round(min(tp), 4), round(max(tp), 4)],
    "unpunctured_ms_min_max": [round(min(tu), 4), round(max(tu), 4)],
    "expansion_bytes_moved": moved, "expansion_budget_us_at_ratio_1_25": round(0.25 * ms_u * 1e3, 1),
    "parity_ok": parity}))
sys.exit(0 if parity else 1)
