#!/usr/bin/env python3
"""Data groups for a whole ensemble: what vit_data_groups_table_dev costs beside the loop of per-stream calls it replaces.
The workloads of bench_dgroups.py: 64 sub-channel streams of 64 kbit/s (192-byte logical frames, 8 slots) at 512 and at
4096 logical frames each, four addresses interleaved packet by packet, groups of 1 ... 8 KB in four-slot packets of 91
bytes, each with a CRC; clean, and with 2 % of the packets lost.  Every stream holds the same bytes.  HIP-event times, the
variants alternating, 9 samples of at least 0.1 s each, median and spread:
  table          vit_data_groups_table_dev on all 64 streams, the data gathered
  loop           64 calls of vit_data_groups_dev, from the same library
  table_1, loop_1  the same for a table of one stream
  chain_table    vit_packet_table_dev (plain packet mode: the streams carry no FEC frames) and then the table call
  chain_loop     vit_packet_table_dev and then the loop
  packet_table   vit_packet_table_dev alone
  device_copy    a device copy of half the bytes the call reads plus writes (a copy reads and writes each byte)
Parity: the table call's output for the first and the last stream against vit_data_groups_host, byte for byte, and every
stream's against the loop's.

usage: bench_dgroup_table.py [samples] [--json FILE]"""
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
from test_dgroup_host import header_bytes, packet  # noqa: E402
from test_packet_host import PACKET_REC_DTYPE, SLOT, make_packet  # noqa: E402

V = _vitpkg.load_package()
assert V.initialize() and V.device_count() >= 1, V.last_error()
args = [a for a in sys.argv[1:]]
json_out = args[args.index("--json") + 1] if "--json" in args else None
samples = int(args[0]) if args and args[0].isdigit() else 9
MIN_MS = 100.0
NSTREAMS, FRAMEBYTES, S = 64, 192, 8
ADDRS = (17, 300, 611, 1021)
rng = np.random.default_rng(2032)


def build_stream(nframes, p_lost):
    """bench_dgroups.py's: nframes * 2 four-slot packets, the groups of the four addresses interleaved"""
    queues = {a: [] for a in ADDRS}
    cont = {a: 0 for a in ADDRS}
    parts = []
    for _ in range(2 * nframes):
        a = ADDRS[int(rng.integers(0, len(ADDRS)))]
        if not queues[a]:
            D = header_bytes(crcf=1, seg=1, ua=1, tidf=1, li=2, payload=rng.integers(0, 256, int(rng.integers(1024, 8193)), dtype=np.uint8),
                             rng=rng)
            queues[a] = [D[k:k + 91] for k in range(0, len(D), 91)]
            queues[a] = [(d, int(k == 0), int(k == len(queues[a]) - 1)) for k, d in enumerate(queues[a])]
        d, first, last = queues[a].pop(0)
        p = packet(rng, 4, a, cont[a], first, last, data=d)
        cont[a] = (cont[a] + 1) & 3
        parts.append(make_packet(rng, 4, 0) if rng.random() < p_lost else p)
    return np.concatenate(parts)


def sample(fn, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / k


def measure(variants):
    calls = {}
    for vn, fn in variants:
        sample(fn, 2)
        calls[vn] = max(1, int(math.ceil(1.2 * MIN_MS / sample(fn, 3))))
    times = {vn: [] for vn, _ in variants}
    for _ in range(samples):
        for vn, fn in variants:
            times[vn].append(sample(fn, calls[vn]))
    return calls, times


def host_call(stream, rec, max_groups, cap):
    dg, sm, data = np.zeros(32 * max_groups, np.uint8), np.zeros(32, np.uint8), np.zeros(max(cap, 1), np.uint8)
    rc = V.lib().vit_data_groups_host(stream.ctypes.data, rec.ctypes.data, rec.size // 8, dg.ctypes.data, max_groups, sm.ctypes.data,
                                      data.ctypes.data, cap)
    assert rc == 0, V.last_error()
    return dg, sm, data


def run(nframes, name, one):
    nslots = nframes * S
    nbytes = nslots * SLOT
    d_all = torch.from_numpy(one).cuda().repeat(NSTREAMS, 1).contiguous()
    d_rec = torch.zeros((NSTREAMS, nslots * PACKET_REC_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    d_srec = torch.zeros((NSTREAMS, 16), dtype=torch.uint8, device="cuda")
    ptab = np.zeros(NSTREAMS, V.PKT_STREAM_DTYPE)
    ptab["offset"] = np.arange(NSTREAMS, dtype=np.uint64) * nbytes
    ptab["framebytes"], ptab["nframes"], ptab["fec"] = FRAMEBYTES, nframes, V.PKT_FEC_NONE
    play = V.packet_table_layout(ptab)
    d_fec = torch.zeros((max(int(play["nfecrec"]), 1) * 16,), dtype=torch.uint8, device="cuda")  # reserved whatever the mode; none written

    def packet_table():
        V.packet_table_dev(d_all, ptab, d_srec, d_fec, d_rec)
    packet_table()
    torch.cuda.synchronize()
    rec0 = d_rec[0].cpu().numpy()
    sm = np.frombuffer(host_call(one, rec0, 0, 0)[1].tobytes(), V.DGROUP_SUM_DTYPE)[0]
    max_groups, cap = int(sm["ngroups"]) + 1, int(sm["data_bytes"])
    w_dg, w_sm, w_data = host_call(one, rec0, max_groups, cap)
    tab = np.zeros(NSTREAMS, V.DG_STREAM_DTYPE)
    tab["offset"], tab["rec_index"] = ptab["offset"], play["rec_index"]
    tab["nslots"], tab["max_groups"], tab["data_capacity"] = nslots, max_groups, cap
    lay = V.data_groups_table_layout(tab)
    assert int(lay["rec_end"]) == NSTREAMS * nslots and int(lay["bytes_end"]) == NSTREAMS * nbytes
    dg_index, data_offset = [int(v) for v in lay["dg_index"]], [int(v) for v in lay["data_offset"]]
    d_dg = torch.zeros((32 * int(lay["ndg"]),), dtype=torch.uint8, device="cuda")
    d_sum = torch.zeros((NSTREAMS, 32), dtype=torch.uint8, device="cuda")
    d_data = torch.zeros((max(int(lay["data_bytes"]), 1),), dtype=torch.uint8, device="cuda")
    dg_k = [d_dg[32 * dg_index[k]:32 * (dg_index[k] + max_groups)] for k in range(NSTREAMS)]
    data_k = [d_data[data_offset[k]:data_offset[k] + max(cap, 1)] for k in range(NSTREAMS)]
    moved = nbytes + 8 * nslots + cap + 32 * max_groups      # read plus written, per stream
    d_src = torch.zeros((NSTREAMS * moved // 2,), dtype=torch.uint8, device="cuda")
    d_dst = torch.zeros_like(d_src)

    def table(n=NSTREAMS):
        V.data_groups_table_dev(d_all, d_rec, tab[:n], d_dg, d_sum, d_data)

    def loop(n=NSTREAMS):
        for k in range(n):
            V.data_groups_dev(d_all[k], d_rec[k], nslots, dg_k[k], max_groups, d_sum[k], data_k[k], cap)

    def chain_table():
        packet_table()
        table()

    def chain_loop():
        packet_table()
        loop()

    calls, times = measure([("table", table), ("loop", loop), ("table_1", lambda: table(1)), ("loop_1", lambda: loop(1)),
                            ("chain_table", chain_table), ("chain_loop", chain_loop), ("packet_table", packet_table),
                            ("device_copy", lambda: d_dst.copy_(d_src))])
    # parity: the table call against the host twin (first and last stream) and against the loop (everything)
    for t in (d_dg, d_sum, d_data):
        t.zero_()
    loop()
    torch.cuda.synchronize()
    want = [t.clone() for t in (d_dg, d_sum, d_data)]
    for t in (d_dg, d_sum, d_data):
        t.zero_()
    table()
    torch.cuda.synchronize()
    ok = all(bool(torch.equal(a, b)) for a, b in zip(want, (d_dg, d_sum, d_data)))
    for k in (0, NSTREAMS - 1):
        ok = ok and dg_k[k].cpu().numpy().tobytes() == w_dg.tobytes() and d_sum[k].cpu().numpy().tobytes() == w_sm.tobytes()
        ok = ok and data_k[k].cpu().numpy()[:cap].tobytes() == w_data[:cap].tobytes()
    med = {k: float(np.median(v)) for k, v in times.items()}
    lo = {k: min(v) for k, v in times.items()}
    hi = {k: max(v) for k, v in times.items()}
    return {"logical_frames": nframes, "input": name, "streams": NSTREAMS, "slots_per_stream": nslots, "groups_per_stream": int(sm["ngroups"]),
            "data_bytes_per_stream": cap, "bytes_read_plus_written": NSTREAMS * moved, "calls_per_sample": calls,
            "ms": {k: round(v, 5) for k, v in med.items()},
            "ms_min_max": {k: [round(lo[k], 5), round(hi[k], 5)] for k in times},
            "loop_over_table": round(med["loop"] / med["table"], 2),
            "loop_over_table_worst": round(lo["loop"] / hi["table"], 2),     # the slowest table sample against the fastest loop sample
            "one_stream_table_minus_loop_us": round(1e3 * (med["table_1"] - med["loop_1"]), 2),
            "chain_loop_over_chain_table": round(med["chain_loop"] / med["chain_table"], 2),
            "table_over_packet_table": round(med["table"] / med["packet_table"], 2),
            "table_over_device_copy": round(med["table"] / med["device_copy"], 2), "parity_ok": bool(ok)}


cases = []
for nf in (512, 4096):
    for name, p_lost in (("clean", 0.0), ("lost_2_percent", 0.02)):
        cases.append(run(nf, name, build_stream(nf, p_lost)))
res = {"samples": samples, "min_sample_ms": MIN_MS, "cases": cases}
line = json.dumps(res)
print(line)
if json_out:
    os.makedirs(os.path.dirname(os.path.abspath(json_out)), exist_ok=True)
    with open(json_out, "w") as f:
        f.write(line + "\n")
sys.exit(0 if all(c["parity_ok"] for c in res["cases"]) else 1)
