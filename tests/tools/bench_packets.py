#!/usr/bin/env python3
"""Packet mode: what the three device calls cost.  64 sub-channel streams of 64 kbit/s (192-byte logical frames, 8 slots)
at 512 and at 4096 logical frames each - one call per stream, as a receiver makes them - clean and with three rows of two
byte errors in every FEC frame.  Every stream holds the same bytes: a period of 8 FEC frames (824 slots) built by
tests/test_packet_host.py, tiled.  HIP-event times, the variants alternating, 9 samples of at least 0.1 s each, median
and spread:
  sync         vit_packet_fec_sync_dev
  fec          vit_packet_fec_dev out of place (the input stays damaged from sample to sample)
  fec_inplace  the same in place (clean input only: clean workgroups write nothing)
  packets      vit_packets_dev
  device_copy  a device copy of the streams: the bytes the out-of-place FEC call reads plus writes
  host_path    what a caller does today: the streams copied to pinned host memory, then vit_packet_fec_frame_host for
               every FEC frame on one thread (host clock around copy + loop; 3 samples)
and a parity check of the FEC output, its records and the packet records against the model on the first period.

usage: bench_packets.py [samples] [--json FILE]"""
import ctypes as C
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
from test_packet_host import (FEC_FRAME_BYTES, FEC_REC_DTYPE, FEC_SLOTS, IDX, PACKET_REC_DTYPE, SLOT,  # noqa: E402
                              build_framed_stream, fec_stream_model, packets_model)

V = _vitpkg.load_package()
assert V.initialize() and V.device_count() >= 1, V.last_error()
args = [a for a in sys.argv[1:]]
json_out = args[args.index("--json") + 1] if "--json" in args else None
samples = int(args[0]) if args and args[0].isdigit() else 9
MIN_MS = 100.0
HOST_SAMPLES = 3
NSTREAMS, FRAMEBYTES, S = 64, 192, 8
PERIOD_FEC = 8
PERIOD_SLOTS = PERIOD_FEC * FEC_SLOTS  # 824 slots = 103 logical frames
rng = np.random.default_rng(2031)

period = {"clean": build_framed_stream(rng, PERIOD_FEC, 0, PERIOD_SLOTS, S)}
bad = period["clean"].copy()
for k in range(PERIOD_FEC):
    for r in rng.permutation(12)[:3]:
        for c in rng.permutation(204)[:2]:
            bad[FEC_FRAME_BYTES * k + IDX[r, c]] ^= int(rng.integers(1, 256))
period["damaged"] = bad
want = {name: (fec_stream_model(p, 0), packets_model(p, FRAMEBYTES)) for name, p in period.items()}


def sample(fn, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / k


def run(nframes, name):
    nslots = nframes * S
    nbytes = nslots * SLOT
    nfec = V.packet_fec_count(nslots, 0)
    one = np.tile(period[name], -(-nslots // PERIOD_SLOTS))[:nbytes]
    d_all = torch.from_numpy(one).cuda().repeat(NSTREAMS, 1).contiguous()
    d_out = torch.zeros_like(d_all)
    d_copy = torch.zeros_like(d_all)
    d_score = torch.zeros((NSTREAMS, FEC_SLOTS), dtype=torch.int32, device="cuda")
    d_fec = torch.zeros((NSTREAMS, nfec * FEC_REC_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    d_rec = torch.zeros((NSTREAMS, nslots * PACKET_REC_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    h_all = torch.zeros((NSTREAMS, nbytes), dtype=torch.uint8).pin_memory()
    h_np = h_all.numpy()
    h_rec = np.zeros(1, FEC_REC_DTYPE)
    host_fn = V.lib().vit_packet_fec_frame_host
    rec_p = h_rec.ctypes.data_as(C.c_void_p)

    def sync():
        for k in range(NSTREAMS):
            V.packet_fec_sync_dev(d_all[k], nslots, d_score[k])

    def fec():
        for k in range(NSTREAMS):
            V.packet_fec_dev(d_all[k], d_out[k], nslots, 0, d_fec[k])

    def fec_inplace():
        for k in range(NSTREAMS):
            V.packet_fec_dev(d_all[k], d_all[k], nslots, 0, d_fec[k])

    def packets():
        for k in range(NSTREAMS):
            V.packets_dev(d_all[k], FRAMEBYTES, nframes, d_rec[k])

    def host_path():
        t0 = time.perf_counter()
        h_all.copy_(d_all, non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        base = h_np.ctypes.data
        for k in range(NSTREAMS):
            for f in range(nfec):
                host_fn(C.c_void_p(base + k * nbytes + f * FEC_FRAME_BYTES), rec_p)
        return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

    variants = [("sync", sync), ("fec", fec), ("packets", packets), ("device_copy", lambda: d_copy.copy_(d_all))]
    if name == "clean":
        variants.insert(2, ("fec_inplace", fec_inplace))
    calls = {}
    for vn, fn in variants:
        sample(fn, 2)
        calls[vn] = max(1, int(math.ceil(1.2 * MIN_MS / sample(fn, 3))))
    times = {vn: [] for vn, _ in variants}
    for _ in range(samples):
        for vn, fn in variants:
            times[vn].append(sample(fn, calls[vn]))
    host = [host_path() for _ in range(HOST_SAMPLES)]
    # parity on the first period of the first and the last stream
    fec()
    packets()
    sync()
    torch.cuda.synchronize()
    (w_bytes, w_fec), w_pkt = want[name]
    n0 = min(PERIOD_FEC, nfec)
    ok = True
    for k in (0, NSTREAMS - 1):
        ok = ok and np.array_equal(d_out[k, :n0 * FEC_FRAME_BYTES].cpu().numpy(), w_bytes[:n0 * FEC_FRAME_BYTES])
        ok = ok and d_fec[k, :n0 * 16].cpu().numpy().tobytes() == w_fec[:n0].tobytes()
        ok = ok and d_rec[k, :PERIOD_SLOTS * 8].cpu().numpy().tobytes() == w_pkt.tobytes()
        ok = ok and int(d_score[k].argmax()) == 0
    med = {k: float(np.median(v)) for k, v in times.items()}
    total = NSTREAMS * nbytes
    d2h, loop = float(np.median([h[0] for h in host])), float(np.median([h[1] for h in host]))
    return {"logical_frames": nframes, "input": name, "streams": NSTREAMS, "bytes": total, "fec_frames": NSTREAMS * nfec,
            "calls_per_sample": calls, "ms": {k: round(v, 5) for k, v in med.items()},
            "ms_min_max": {k: [round(min(v), 5), round(max(v), 5)] for k, v in times.items()},
            "host_path_ms": {"d2h_copy": round(d2h, 4), "fec_frame_host_loop": round(loop, 3), "total": round(d2h + loop, 3),
                             "total_min_max": [round(min(a + b for a, b in host), 3), round(max(a + b for a, b in host), 3)]},
            "fec_GBps_read": round(total / med["fec"] / 1e6, 2),
            "packets_GBps_read": round(total / med["packets"] / 1e6, 2),
            "fec_over_device_copy": round(med["fec"] / med["device_copy"], 2),
            "packets_over_device_copy": round(med["packets"] / med["device_copy"], 2),
            "sync_over_device_copy": round(med["sync"] / med["device_copy"], 2),
            "host_path_over_fec": round((d2h + loop) / med["fec"], 1), "parity_ok": bool(ok)}


res = {"samples": samples, "min_sample_ms": MIN_MS, "host_samples": HOST_SAMPLES,
       "cases": [run(nf, name) for nf in (512, 4096) for name in ("clean", "damaged")]}
line = json.dumps(res)
print(line)
if json_out:
    os.makedirs(os.path.dirname(os.path.abspath(json_out)), exist_ok=True)
    with open(json_out, "w") as f:
        f.write(line + "\n")
sys.exit(0 if all(c["parity_ok"] for c in res["cases"]) else 1)
