#!/usr/bin/env python3
"""DAB+ access units: what the AU pass costs behind the chain.  16384 superframes at RSDims 24 (64 distinct ones of
built AUs tiled, 3 dB, punctured).  HIP-event times, the variants alternating, 9 samples of at least 0.1 s each, median:
  (a) vit_dabplus_punctured_superframes_dev alone (the baseline)
  (b) the same call followed by vit_dabplus_aus_dev on d_rs_out with d_ret
  (c) vit_dabplus_aus_dev alone
  (d) a device copy of the bytes it reads (110*RSDims per superframe), for scale
  (e) what a caller did before: the copy of d_rs_out to pinned host memory
and a parity check of the table against the model.  The kernels' own times come from one
`rocprofv3 --kernel-trace --stats` run of this script (profiles/r12_au_kstats.csv).

usage: bench_au.py [samples] [--json FILE]
       bench_au.py profile          (5 x (chain, AU pass) and nothing else: the run to trace)"""
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
from bench import rs_encode_columns  # noqa: E402
from test_au_host import AU_DTYPE, AU_OK, PARAM, au_table_model, make_superframe, random_starts  # noqa: E402
from test_dab_host import scramble  # noqa: E402
from test_gpu_dab import dabplus_symbols  # noqa: E402
from test_punct_host import KEEP_24, KEEP_TAIL_12, depuncture, puncture  # noqa: E402

V = _vitpkg.load_package()
O = _vitpkg.load_oracle()
O.build()
assert V.initialize() and V.device_count() >= 1, V.last_error()
V.set_renorm_ge(0)
args = [a for a in sys.argv[1:]]
json_out = args[args.index("--json") + 1] if "--json" in args else None
samples = int(args[0]) if args and args[0].isdigit() else 9
MIN_MS = 100.0
rng = np.random.default_rng(2027)

rsdims, nsf, base_sf = 24, 16384, 64
fb, L = 192 * rsdims, 110 * rsdims
nums = [(2, 3, 4, 6)[i % 4] for i in range(base_sf)]
pay = np.stack([make_superframe(rng, rsdims, PARAM[n], random_starts(rng, rsdims, n)) for n in nums])
cw = rs_encode_columns(pay.reshape(base_sf, 110, rsdims).transpose(1, 0, 2).reshape(110, base_sf * rsdims))
sf = np.ascontiguousarray(cw.reshape(120, base_sf, rsdims).transpose(1, 0, 2).reshape(base_sf, 120 * rsdims))
segs = [(fb, KEEP_24), (6, KEEP_TAIL_12)]
punct = puncture(dabplus_symbols(O, rng, sf, rsdims, ["3dB"] * base_sf), segs, fb)
work_ref = scramble(O.decode_batch(fb, depuncture(punct, segs, fb, 128), nthreads=16), fb).reshape(base_sf, -1)
ret_ref, out_ref = O.rs_check_batch(work_ref, rsdims)
want = au_table_model(out_ref, rsdims, ret_ref)

reps = nsf // base_sf
d_in = torch.from_numpy(punct).cuda().repeat(reps, 1).contiguous()
d_work = torch.zeros((nsf, 120 * rsdims), dtype=torch.uint8, device="cuda")
d_out = torch.zeros((nsf, L), dtype=torch.uint8, device="cuda")
d_ret = torch.zeros(nsf, dtype=torch.int32, device="cuda")
d_fire = torch.zeros(nsf, dtype=torch.uint8, device="cuda")
d_au = torch.zeros((nsf, AU_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
d_copy = torch.zeros_like(d_out)
h_out = torch.zeros((nsf, L), dtype=torch.uint8).pin_memory()


def chain():
    V.dabplus_punctured_superframes_dev(d_in, segs, d_work, d_out, d_ret, rsdims, nsf, d_fire_ok=d_fire)


def aus():
    V.dabplus_aus_dev(d_out, rsdims, nsf, d_au, d_ret=d_ret)


def chain_aus():
    chain()
    aus()


VARIANTS = [("chain", chain), ("chain_plus_aus", chain_aus), ("aus", aus),
            ("device_copy", lambda: d_copy.copy_(d_out)), ("d2h_copy", lambda: h_out.copy_(d_out, non_blocking=True))]


def sample(fn, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / k


if "profile" in args:
    for _ in range(5):
        chain_aus()
    torch.cuda.synchronize()
    sys.exit(0)

calls = {}
for name, fn in VARIANTS:  # code objects, scratch growth; then as many calls per sample as fill MIN_MS
    sample(fn, 3)
    calls[name] = max(1, int(math.ceil(1.2 * MIN_MS / sample(fn, 5))))
times = {name: [] for name, _ in VARIANTS}
for _ in range(samples):
    for name, fn in VARIANTS:
        times[name].append(sample(fn, calls[name]))

chain_aus()
torch.cuda.synchronize()
parity = bool((d_au.view(reps, base_sf, -1) ==
               torch.from_numpy(want.view(np.uint8).reshape(base_sf, -1)).cuda().unsqueeze(0)).all())
med = {k: float(np.median(v)) for k, v in times.items()}
a, b = med["chain"], med["chain_plus_aus"]
res = {"nsf": nsf, "rsdims": rsdims, "samples": samples, "min_sample_ms": MIN_MS, "calls_per_sample": calls,
       "ms": {k: round(v, 5) for k, v in med.items()},
       "ms_min_max": {k: [round(min(v), 5), round(max(v), 5)] for k, v in times.items()},
       "chain_samples_ms": [round(x, 5) for x in times["chain"]],
       "aus_behind_chain_ms": round(b - a, 5), "aus_behind_chain_percent": round(100.0 * (b - a) / a, 3),
       "chain_spread_percent": round(100.0 * (max(times["chain"]) - min(times["chain"])) / a, 3),
       "bytes_read": nsf * L, "aus_alone_GBps": round(nsf * L / med["aus"] / 1e6, 1),
       "device_copy_GBps_read_plus_write": round(2 * nsf * L / med["device_copy"] / 1e6, 1),
       "superframes_ok_in_sample": int((want["status"] == AU_OK).sum()),
       "aus_with_good_crc_in_sample": int(sum(bin(int(x)).count("1") for x in want["crc_ok"])),
       "rs_failed_in_sample": int((ret_ref < 0).sum()), "parity_ok": parity}
line = json.dumps(res)
print(line)
if json_out:
    os.makedirs(os.path.dirname(os.path.abspath(json_out)), exist_ok=True)
    with open(json_out, "w") as f:
        f.write(line + "\n")
sys.exit(0 if parity else 1)
