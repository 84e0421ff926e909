#!/usr/bin/env python3
"""Packet mode for a whole ensemble: what vit_packet_table_dev costs beside the per-stream calls it replaces.  The streams
of bench_packets.py: 64 sub-channel streams of 64 kbit/s (192-byte logical frames, 8 slots) at 512 and at 4096 logical
frames each, clean and with three rows of two byte errors in every FEC frame, every stream the same tiled period of 8 FEC
frames.  Everything works in place on one work buffer; with damaged input every timed call is preceded by the device copy
that restores the damage (restore_in_timed_loop), so that each call finds rows to correct.  HIP-event times, the variants
alternating, 9 samples of at least 0.1 s each, median and spread:
  table          (a) vit_packet_table_dev, FEC_SEARCH on all 64 streams, scores in the caller's d_score
  loop           (b) the recipe it replaces: per stream vit_packet_fec_sync_dev, argmax with its copy to the host,
                     vit_packet_fec_dev in place, vit_packets_dev
  loop_known     (c) the same loop with the phases known: no sync call and no round trip
  device_copy    (d) a device copy of the streams: the bytes read plus written
  table_1, loop_1  (e) (a) and (b) for a table of one stream
The per-stream calls are those of --parent-lib (the parent commit's libviterbi.so, loaded beside this one in the same
process) or, without it, this library's.  A parity check compares the table call's bytes and records with the loop's.

usage: bench_packet_table.py [samples] [--parent-lib FILE] [--json FILE]"""
import ctypes as C
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
from test_packet_host import FEC_FRAME_BYTES, FEC_REC_DTYPE, FEC_SLOTS, IDX, PACKET_REC_DTYPE, SLOT, build_framed_stream  # noqa: E402

V = _vitpkg.load_package()
assert V.initialize() and V.device_count() >= 1, V.last_error()
args = [a for a in sys.argv[1:]]
json_out = args[args.index("--json") + 1] if "--json" in args else None
parent_path = args[args.index("--parent-lib") + 1] if "--parent-lib" in args else None
samples = int(args[0]) if args and args[0].isdigit() else 9
MIN_MS = 100.0
NSTREAMS, FRAMEBYTES, S = 64, 192, 8
PERIOD_FEC = 8
PERIOD_SLOTS = PERIOD_FEC * FEC_SLOTS
rng = np.random.default_rng(2031)

L = V.lib()
vp = C.c_void_p
if parent_path:
    P = C.CDLL(os.path.abspath(parent_path))
    P.vit_packet_fec_sync_dev.argtypes = [vp, C.c_int64, vp, vp]
    P.vit_packet_fec_dev.argtypes = [vp, vp, C.c_int64, C.c_uint32, vp, vp]
    P.vit_packets_dev.argtypes = [vp, C.c_uint32, C.c_int64, vp, vp]
    assert not hasattr(P, "vit_packet_table_dev"), "--parent-lib must be the parent commit's library"
else:
    P = L

period = {"clean": build_framed_stream(rng, PERIOD_FEC, 0, PERIOD_SLOTS, S)}
bad = period["clean"].copy()
for k in range(PERIOD_FEC):
    for r in rng.permutation(12)[:3]:
        for c in rng.permutation(204)[:2]:
            bad[FEC_FRAME_BYTES * k + IDX[r, c]] ^= int(rng.integers(1, 256))
period["damaged"] = bad


def sample(fn, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / k


def ok(rc):
    assert rc == 0, V.last_error()


def run(nframes, name):
    nslots = nframes * S
    nbytes = nslots * SLOT
    nfec_max = nslots // FEC_SLOTS
    restore = name == "damaged"
    one = np.tile(period[name], -(-nslots // PERIOD_SLOTS))[:nbytes]
    d_src = torch.from_numpy(one).cuda().repeat(NSTREAMS, 1).contiguous()
    d_work = d_src.clone()
    d_copy = torch.zeros_like(d_src)
    d_score = torch.zeros((NSTREAMS, FEC_SLOTS), dtype=torch.int32, device="cuda")
    d_srec = torch.zeros((NSTREAMS, 16), dtype=torch.uint8, device="cuda")
    d_fec = torch.zeros((NSTREAMS, nfec_max * FEC_REC_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    d_rec = torch.zeros((NSTREAMS, nslots * PACKET_REC_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    tab = np.zeros(NSTREAMS, V.PKT_STREAM_DTYPE)
    tab["offset"] = np.arange(NSTREAMS, dtype=np.uint64) * nbytes
    tab["framebytes"], tab["nframes"], tab["fec"] = FRAMEBYTES, nframes, V.PKT_FEC_SEARCH
    lay = V.packet_table_layout(tab)
    assert int(lay["nrec"]) == NSTREAMS * nslots and int(lay["nfecrec"]) == NSTREAMS * nfec_max
    tab_p = tab.ctypes.data
    work, srec, fec, rec, score = (t.data_ptr() for t in (d_work, d_srec, d_fec, d_rec, d_score))
    fec_stride, rec_stride = d_fec.shape[1], d_rec.shape[1]

    def table(n=NSTREAMS):
        if restore:
            d_work[:n].copy_(d_src[:n])
        ok(L.vit_packet_table_dev(work, tab_p, n, srec, fec, rec, score, None))

    def loop(n=NSTREAMS, known=False):
        if restore:
            d_work[:n].copy_(d_src[:n])
        for k in range(n):
            s = work + k * nbytes
            phase = 0
            if not known:
                ok(P.vit_packet_fec_sync_dev(s, nslots, score + 4 * FEC_SLOTS * k, None))
                phase = int(d_score[k].argmax())
            ok(P.vit_packet_fec_dev(s, s, nslots, phase, fec + k * fec_stride, None))
            ok(P.vit_packets_dev(s, FRAMEBYTES, nframes, rec + k * rec_stride, None))

    variants = [("table", table), ("loop", loop), ("loop_known", lambda: loop(known=True)), ("device_copy", lambda: d_copy.copy_(d_src)),
                ("table_1", lambda: table(1)), ("loop_1", lambda: loop(1))]
    calls = {}
    for vn, fn in variants:
        sample(fn, 2)
        calls[vn] = max(1, int(math.ceil(1.2 * MIN_MS / sample(fn, 3))))
    times = {vn: [] for vn, _ in variants}
    for _ in range(samples):
        for vn, fn in variants:
            times[vn].append(sample(fn, calls[vn]))
    # parity: the table call against the loop, every byte of every output
    d_fec.fill_(0)
    loop()
    torch.cuda.synchronize()
    want = [t.clone() for t in (d_work, d_fec, d_rec, d_score)]
    d_fec.fill_(0)
    table()
    torch.cuda.synchronize()
    same = all(bool(torch.equal(a, b)) for a, b in zip(want, (d_work, d_fec, d_rec, d_score)))
    sr = d_srec.cpu().numpy().view(V.PKT_STREAM_REC_DTYPE).reshape(-1)
    same = same and (sr["phase"] == 0).all() and (sr["nfec"] == nfec_max).all() and bool(torch.equal(d_work, d_src) == (name == "clean"))
    med = {k: float(np.median(v)) for k, v in times.items()}
    return {"logical_frames": nframes, "input": name, "streams": NSTREAMS, "bytes": NSTREAMS * nbytes, "fec_frames": NSTREAMS * nfec_max,
            "restore_in_timed_loop": restore, "calls_per_sample": calls, "ms": {k: round(v, 5) for k, v in med.items()},
            "ms_min_max": {k: [round(min(v), 5), round(max(v), 5)] for k, v in times.items()},
            "loop_over_table": round(med["loop"] / med["table"], 2), "loop_known_over_table": round(med["loop_known"] / med["table"], 2),
            "table_over_device_copy": round(med["table"] / med["device_copy"], 2),
            "one_stream_table_minus_loop_us": round(1e3 * (med["table_1"] - med["loop_1"]), 2),
            "one_stream_loop_over_table": round(med["loop_1"] / med["table_1"], 2), "parity_ok": bool(same)}


res = {"samples": samples, "min_sample_ms": MIN_MS, "per_stream_calls": "parent library" if parent_path else "this library",
       "cases": [run(nf, name) for nf in (512, 4096) for name in ("clean", "damaged")]}
line = json.dumps(res)
print(line)
if json_out:
    os.makedirs(os.path.dirname(os.path.abspath(json_out)), exist_ok=True)
    with open(json_out, "w") as f:
        f.write(line + "\n")
sys.exit(0 if all(c["parity_ok"] for c in res["cases"]) else 1)
