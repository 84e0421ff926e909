#!/usr/bin/env python3
"""Multiplex configuration: what vit_mci_fibs_dev costs.  49152 FIBs (the FICs of 4096 mode-I transmission frames; every
FIB with a valid CRC, a period of 384 well-formed FIBs from the builders of tests/test_mci_host.py, tiled) at G = 12 (a
transmission frame a group) and at G = 4096.  HIP-event times, the variants alternating, 9 samples of at least 0.1 s each,
median and spread:
  mci          vit_mci_fibs_dev with flags and status bytes
  device_copy  a device copy of as many bytes as the call reads plus writes (FIBs, flags, records, status)
  host_path    what a caller does today: d_fibs and the flags copied to pinned host memory, then vit_mci_fibs_host on one
               thread (host clock around copy + call; 3 samples)
  fic          vit_decode_fic_dev alone on the same FIBs through the mother code, punctured (noise-free)
  fic_mci      the same followed by vit_mci_fibs_dev on its outputs, on the same stream
and a parity check of the device records against vit_mci_fibs_host.

usage: bench_mci.py [samples] [--json FILE]"""
import json
import math
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import _vitpkg  # noqa: E402
from test_dab_host import scramble  # noqa: E402
from test_mci_host import random_fibs  # noqa: E402
from test_punct_host import fic_segments, puncture  # noqa: E402

V = _vitpkg.load_package()
O = _vitpkg.load_oracle()
assert V.initialize() and V.device_count() >= 1, V.last_error()
args = [a for a in sys.argv[1:]]
json_out = args[args.index("--json") + 1] if "--json" in args else None
samples = int(args[0]) if args and args[0].isdigit() else 9
MIN_MS = 100.0
HOST_SAMPLES = 3
NFIBS, PERIOD, FRAMEBITS = 49152, 384, 768
SREC, GREC = V.MCI_SUBCH_DTYPE.itemsize, V.MCI_GROUP_DTYPE.itemsize
rng = np.random.default_rng(2032)

period = random_fibs(rng, PERIOD)                       # 128 FIC frames of three FIBs
frames = period.reshape(PERIOD // 3, 96)
bits = np.unpackbits(scramble(frames, FRAMEBITS), axis=1)
sym = (np.stack([O.encode(b) for b in bits]) * 255).astype(np.uint8)
punct = puncture(sym, fic_segments(), FRAMEBITS)
NFRAMES = NFIBS // 3
d_fibs = torch.from_numpy(period.reshape(-1)).cuda().repeat(NFIBS // PERIOD).contiguous()
d_ok = torch.ones(NFIBS, dtype=torch.uint8, device="cuda")
d_st = torch.zeros(NFIBS, dtype=torch.uint8, device="cuda")
d_in = torch.from_numpy(punct).cuda().repeat(NFRAMES // punct.shape[0], 1).contiguous()
d_f = torch.zeros(NFIBS * 32, dtype=torch.uint8, device="cuda")
d_fok = torch.zeros(NFIBS, dtype=torch.uint8, device="cuda")
h_fibs = torch.zeros(NFIBS * 32, dtype=torch.uint8).pin_memory()
h_ok = torch.zeros(NFIBS, dtype=torch.uint8).pin_memory()


def sample(fn, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / k


def run(G):
    ng = -(-NFIBS // G)
    d_sub = torch.zeros(ng * 64 * SREC, dtype=torch.uint8, device="cuda")
    d_grp = torch.zeros(ng * GREC, dtype=torch.uint8, device="cuda")
    moved = NFIBS * 32 + NFIBS + d_sub.numel() + d_grp.numel() + NFIBS   # read: FIBs, flags; written: records, status
    d_a = torch.zeros((moved + 1) // 2, dtype=torch.uint8, device="cuda")
    d_b = torch.zeros_like(d_a)

    def mci():
        V.mci_fibs_dev(d_fibs, NFIBS, G, d_sub, d_grp, d_ok, d_st)

    def fic():
        V.decode_fic_dev(d_in, d_f, d_fok, FRAMEBITS, NFRAMES, fic_segments())

    def fic_mci():
        fic()
        V.mci_fibs_dev(d_f, NFIBS, G, d_sub, d_grp, d_fok, d_st)

    def host_path():
        t0 = time.perf_counter()
        h_fibs.copy_(d_fibs, non_blocking=True)
        h_ok.copy_(d_ok, non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        V.mci_fibs_host(h_fibs.numpy(), G, h_ok.numpy())
        return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

    variants = [("mci", mci), ("device_copy", lambda: d_b.copy_(d_a)), ("fic", fic), ("fic_mci", fic_mci)]
    calls = {}
    for vn, fn in variants:
        sample(fn, 2)
        calls[vn] = max(1, int(math.ceil(1.2 * MIN_MS / sample(fn, 3))))
    times = {vn: [] for vn, _ in variants}
    for _ in range(samples):
        for vn, fn in variants:
            times[vn].append(sample(fn, calls[vn]))
    host = [host_path() for _ in range(HOST_SAMPLES)]
    # parity: the chain's FIBs are the period again, and both device results are the host twin's
    fic_mci()
    torch.cuda.synchronize()
    chain = (d_sub.cpu().numpy().tobytes(), d_grp.cpu().numpy().tobytes(), d_st.cpu().numpy().tobytes())
    mci()
    torch.cuda.synchronize()
    alone = (d_sub.cpu().numpy().tobytes(), d_grp.cpu().numpy().tobytes(), d_st.cpu().numpy().tobytes())
    want = tuple(a.tobytes() for a in V.mci_fibs_host(d_fibs.cpu().numpy(), G, d_ok.cpu().numpy()))
    ok = alone == want and chain == want and bool(d_fok.all()) and bool((d_f == d_fibs).all())
    med = {k: float(np.median(v)) for k, v in times.items()}
    d2h, call = float(np.median([h[0] for h in host])), float(np.median([h[1] for h in host]))
    return {"G": G, "nfibs": NFIBS, "groups": ng, "bytes_read_plus_written": moved, "calls_per_sample": calls,
            "ms": {k: round(v, 5) for k, v in med.items()},
            "ms_min_max": {k: [round(min(v), 5), round(max(v), 5)] for k, v in times.items()},
            "host_path_ms": {"d2h_copy": round(d2h, 4), "mci_fibs_host": round(call, 3), "total": round(d2h + call, 3),
                             "total_min_max": [round(min(a + b for a, b in host), 3), round(max(a + b for a, b in host), 3)]},
            "mci_GBps_moved": round(moved / med["mci"] / 1e6, 2),
            "mci_over_device_copy": round(med["mci"] / med["device_copy"], 2),
            "host_path_over_mci": round((d2h + call) / med["mci"], 1),
            "fic_mci_over_fic": round(med["fic_mci"] / med["fic"], 4), "parity_ok": bool(ok)}


res = {"samples": samples, "min_sample_ms": MIN_MS, "host_samples": HOST_SAMPLES, "cases": [run(G) for G in (12, 4096)]}
line = json.dumps(res)
print(line)
if json_out:
    os.makedirs(os.path.dirname(os.path.abspath(json_out)), exist_ok=True)
    with open(json_out, "w") as f:
        f.write(line + "\n")
sys.exit(0 if all(c["parity_ok"] for c in res["cases"]) else 1)
