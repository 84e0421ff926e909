#!/usr/bin/env python3
"""Service directory: what vit_mci_dir_dev costs.  49152 FIBs (the FICs of 4096 mode-I transmission frames; every FIB
with a valid CRC) of a multiplex as it is on air - 18 audio services and two packet-mode services in one sub-channel, the
services of FIG 0/2 four to a FIG in rotation, FIG 0/3 with the two packet components, FIG 0/0 and 0/1, the ensemble label
and the twenty service labels one to a FIB in rotation: a period of 240 FIBs from the builders of the tests, tiled - at
G = 12 (a transmission frame a group) and at G = 4096.  HIP-event times, the variants alternating, 9 samples of at least
0.1 s each, median and spread:
  dir          vit_mci_dir_dev with flags and status bytes
  mci          vit_mci_fibs_dev alone on the same FIBs
  mci_dir      the two one after the other on the same stream
  device_copy  a device copy of as many bytes as vit_mci_dir_dev reads plus writes (FIBs, flags, records, status)
  host_path    the FIBs and the flags copied to pinned host memory, then vit_mci_dir_host on one thread (host clock around
               copy + call; 3 samples)
and a parity check of the device records against vit_mci_dir_host.

usage: bench_mci_dir.py [samples] [--json FILE] [--rehearse]   (--rehearse: no GPU; builds the input, runs the host twin)"""
import json
import math
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import _vitpkg  # noqa: E402
from test_mci_dir_host import fig1, fig03, loc_entry, pcomp  # noqa: E402
from test_mci_host import comp, fib, fig0, fig00, fig01_long, fig02_service  # noqa: E402

V = _vitpkg.load_package()
args = [a for a in sys.argv[1:]]
json_out = args[args.index("--json") + 1] if "--json" in args else None
rehearse = "--rehearse" in args
samples = int(args[0]) if args and args[0].isdigit() else 9
MIN_MS = 100.0
HOST_SAMPLES = 3
NFIBS, PERIOD = 49152, 240
NSERVICES = 20


def multiplex_period():
    """240 FIBs: FIB i carries, by i % 4, services (and the packet locations), a label, the sub-channels, the ensemble"""
    svcs = [fig02_service(0xD101 + k, [comp(0, 63, 1 + k)]) for k in range(NSERVICES - 2)]
    svcs += [fig02_service(0xD1F1, [pcomp(0x101)]), fig02_service(0xD1F2, [pcomp(0x102, 0)])]
    names = ["Station %02d" % k for k in range(NSERVICES - 2)] + ["Slideshow", "Traffic data"]
    sids = [0xD101 + k for k in range(NSERVICES - 2)] + [0xD1F1, 0xD1F2]
    locs = fig03(loc_entry(0x101, 19, 5, dscty=60), loc_entry(0x102, 19, 700, dscty=5))
    out = []
    for i in range(PERIOD):
        r, c = i % 4, i // 4
        if r == 0:
            four = b"".join(svcs[(4 * c + j) % NSERVICES] for j in range(4))
            out.append(fib(fig0(2, 0, 0, 0, four), locs) if len(four) + 2 + len(locs) <= 30 else fib(fig0(2, 0, 0, 0, four)))
        elif r == 1:
            out.append(fib(fig1(1, sids[c % NSERVICES], names[c % NSERVICES])))
        elif r == 2:
            out.append(fib(fig00(0xD220, 0, 0, (4 * c) % 5000),
                           fig0(1, 0, 0, 0, b"".join(fig01_long(1 + (5 * c + j) % 19, 40 * ((5 * c + j) % 19), 0, 2, 36) for j in range(5)))))
        else:
            out.append(fib(fig1(0, 0xD220, "The Ensemble")) if c % 3 == 0 else fib(locs, fig0(2, 0, 0, 0, svcs[18] + svcs[19])))
    return np.stack(out)


period = multiplex_period()
if rehearse:
    svc, pkt, d, st = V.mci_dir_host(period, 12)
    full = V.mci_dir_host(period, PERIOD)[2][0]
    print(json.dumps({"rehearsal": True, "nsvc": int(full["nsvc"]), "npkt": int(full["npkt"]), "labelled": int((V.mci_dir_host(period, PERIOD)[0][0]["flags"] & 1).sum()),
                      "malformed": int((st & 2).sum()), "groups_of_12": len(d)}))
    sys.exit(0)

import torch  # noqa: E402

assert V.initialize() and V.device_count() >= 1, V.last_error()
SREC, GREC = V.MCI_SUBCH_DTYPE.itemsize, V.MCI_GROUP_DTYPE.itemsize
VREC, PREC, DREC = V.MCI_SERVICE_DTYPE.itemsize, V.MCI_PKTCOMP_DTYPE.itemsize, V.MCI_DIR_DTYPE.itemsize
reps = -(-NFIBS // PERIOD)
d_fibs = torch.from_numpy(period.reshape(-1)).cuda().repeat(reps)[:NFIBS * 32].contiguous()
d_ok = torch.ones(NFIBS, dtype=torch.uint8, device="cuda")
d_st = torch.zeros(NFIBS, dtype=torch.uint8, device="cuda")
d_st2 = torch.zeros(NFIBS, dtype=torch.uint8, device="cuda")
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
    d_svc = torch.zeros(ng * 64 * VREC, dtype=torch.uint8, device="cuda")
    d_pkt = torch.zeros(ng * 64 * PREC, dtype=torch.uint8, device="cuda")
    d_dir = torch.zeros(ng * DREC, dtype=torch.uint8, device="cuda")
    d_sub = torch.zeros(ng * 64 * SREC, dtype=torch.uint8, device="cuda")
    d_grp = torch.zeros(ng * GREC, dtype=torch.uint8, device="cuda")
    moved = NFIBS * 32 + NFIBS + d_svc.numel() + d_pkt.numel() + d_dir.numel() + NFIBS   # read: FIBs, flags; written: records, status
    d_a = torch.zeros((moved + 1) // 2, dtype=torch.uint8, device="cuda")
    d_b = torch.zeros_like(d_a)

    def dir_():
        V.mci_dir_dev(d_fibs, NFIBS, G, d_svc, d_pkt, d_dir, d_ok, d_st)

    def mci():
        V.mci_fibs_dev(d_fibs, NFIBS, G, d_sub, d_grp, d_ok, d_st2)

    def mci_dir():
        mci()
        dir_()

    def host_path():
        t0 = time.perf_counter()
        h_fibs.copy_(d_fibs, non_blocking=True)
        h_ok.copy_(d_ok, non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        V.mci_dir_host(h_fibs.numpy(), G, h_ok.numpy())
        return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

    variants = [("dir", dir_), ("mci", mci), ("mci_dir", mci_dir), ("device_copy", lambda: d_b.copy_(d_a))]
    calls = {}
    for vn, fn in variants:
        sample(fn, 2)
        calls[vn] = max(1, int(math.ceil(1.2 * MIN_MS / sample(fn, 3))))
    times = {vn: [] for vn, _ in variants}
    for _ in range(samples):
        for vn, fn in variants:
            times[vn].append(sample(fn, calls[vn]))
    host = [host_path() for _ in range(HOST_SAMPLES)]
    dir_()
    torch.cuda.synchronize()
    got = (d_svc.cpu().numpy().tobytes(), d_pkt.cpu().numpy().tobytes(), d_dir.cpu().numpy().tobytes(), d_st.cpu().numpy().tobytes())
    want = V.mci_dir_host(d_fibs.cpu().numpy(), G, d_ok.cpu().numpy())
    ok = got == tuple(a.tobytes() for a in want)
    med = {k: float(np.median(v)) for k, v in times.items()}
    d2h, call = float(np.median([h[0] for h in host])), float(np.median([h[1] for h in host]))
    return {"G": G, "nfibs": NFIBS, "groups": ng, "bytes_read_plus_written": moved, "calls_per_sample": calls,
            "nsvc_last_group": int(want[2][-1]["nsvc"]), "npkt_last_group": int(want[2][-1]["npkt"]),
            "ms": {k: round(v, 5) for k, v in med.items()},
            "ms_min_max": {k: [round(min(v), 5), round(max(v), 5)] for k, v in times.items()},
            "host_path_ms": {"d2h_copy": round(d2h, 4), "mci_dir_host": round(call, 3), "total": round(d2h + call, 3),
                             "total_min_max": [round(min(a + b for a, b in host), 3), round(max(a + b for a, b in host), 3)]},
            "dir_GBps_moved": round(moved / med["dir"] / 1e6, 2),
            "dir_over_device_copy": round(med["dir"] / med["device_copy"], 2),
            "dir_over_mci": round(med["dir"] / med["mci"], 2),
            "mci_dir_over_sum": round(med["mci_dir"] / (med["mci"] + med["dir"]), 3),
            "host_path_over_dir": round((d2h + call) / med["dir"], 2), "parity_ok": bool(ok)}


res = {"samples": samples, "min_sample_ms": MIN_MS, "host_samples": HOST_SAMPLES, "period_fibs": PERIOD,
       "cases": [run(G) for G in (12, 4096)]}
line = json.dumps(res)
print(line)
if json_out:
    os.makedirs(os.path.dirname(os.path.abspath(json_out)), exist_ok=True)
    with open(json_out, "w") as f:
        f.write(line + "\n")
sys.exit(0 if all(c["parity_ok"] for c in res["cases"]) else 1)
