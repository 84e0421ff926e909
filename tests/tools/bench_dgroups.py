#!/usr/bin/env python3
"""MSC data groups on the device: what vit_data_groups_dev costs.  64 sub-channel streams of 64 kbit/s (192-byte logical
frames, 8 slots) at 512 and at 4096 logical frames each - one call per stream, as a receiver makes them.  Content: four
addresses interleaved packet by packet, groups of 1 ... 8 KB in four-slot packets of 91 bytes, each with a CRC; clean, and
with 2 % of the packets lost (padding in their place).  Every stream holds the same bytes.  HIP-event times, the variants
alternating, 9 samples of at least 0.1 s each, median and spread:
  dgroups       vit_data_groups_dev with the data gathered
  records_only  the same with d_data NULL
  packets       vit_packets_dev on the same streams (a call of the same launch-bound kind)
  device_copy   a device copy of half the bytes the call reads plus writes (a copy reads and writes each byte)
  host_path     what a caller did before: records and streams copied to pinned host memory, then vit_data_groups_host
                for every stream on one thread (host clock around copy + loop; 3 samples)
and worst_case: one stream of 4096 frames in which all 1021 data addresses occur (one-packet groups), one call.
Parity: the first and the last stream's output against the host twin, byte for byte, and for 512 frames the host twin
against the Python model of tests/test_dgroup_host.py.

usage: bench_dgroups.py [samples] [--json FILE]"""
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
from test_dgroup_host import dgroups_model, header_bytes, packet  # noqa: E402
from test_packet_host import PACKET_REC_DTYPE, SLOT, make_packet  # noqa: E402

V = _vitpkg.load_package()
assert V.initialize() and V.device_count() >= 1, V.last_error()
args = [a for a in sys.argv[1:]]
json_out = args[args.index("--json") + 1] if "--json" in args else None
samples = int(args[0]) if args and args[0].isdigit() else 9
MIN_MS = 100.0
HOST_SAMPLES = 3
NSTREAMS, FRAMEBYTES, S = 64, 192, 8
ADDRS = (17, 300, 611, 1021)
rng = np.random.default_rng(2032)


def build_stream(nframes, p_lost):
    """nframes * 2 four-slot packets: the groups of the four addresses, interleaved"""
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


def worst_stream(nframes):
    """one-slot packets, each a group of its own, over all 1021 data addresses in turn"""
    return np.concatenate([packet(rng, 1, 1 + k % 1021, 0, 1, 1, useful=19) for k in range(nframes * S)])


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


def run(nframes, name, one, nstreams):
    nslots = nframes * S
    nbytes = nslots * SLOT
    d_all = torch.from_numpy(one).cuda().repeat(nstreams, 1).contiguous()
    d_rec = torch.zeros((nstreams, nslots * PACKET_REC_DTYPE.itemsize), dtype=torch.uint8, device="cuda")

    def packets():
        for k in range(nstreams):
            V.packets_dev(d_all[k], FRAMEBYTES, nframes, d_rec[k])
    packets()
    torch.cuda.synchronize()
    rec0 = d_rec[0].cpu().numpy()
    max_groups = nslots
    sm = np.frombuffer(host_call(one, rec0, 0, 0)[1].tobytes(), V.DGROUP_SUM_DTYPE)[0]
    max_groups, cap = int(sm["ngroups"]) + 1, int(sm["data_bytes"])
    w_dg, w_sm, w_data = host_call(one, rec0, max_groups, cap)
    d_dg = torch.zeros((nstreams, 32 * max_groups), dtype=torch.uint8, device="cuda")
    d_sum = torch.zeros((nstreams, 32), dtype=torch.uint8, device="cuda")
    d_data = torch.zeros((nstreams, max(cap, 1)), dtype=torch.uint8, device="cuda")
    moved = nbytes + 8 * nslots + cap + 32 * max_groups      # read plus written, per stream
    d_src = torch.zeros((nstreams * moved // 2,), dtype=torch.uint8, device="cuda")
    d_dst = torch.zeros_like(d_src)
    h_all = torch.zeros((nstreams, nbytes), dtype=torch.uint8).pin_memory()
    h_rec = torch.zeros((nstreams, 8 * nslots), dtype=torch.uint8).pin_memory()
    h_np, h_rnp = h_all.numpy(), h_rec.numpy()

    def dgroups():
        for k in range(nstreams):
            V.data_groups_dev(d_all[k], d_rec[k], nslots, d_dg[k], max_groups, d_sum[k], d_data[k], cap)

    def records_only():
        for k in range(nstreams):
            V.data_groups_dev(d_all[k], d_rec[k], nslots, d_dg[k], max_groups, d_sum[k], None, 0)

    def host_path():
        t0 = time.perf_counter()
        h_all.copy_(d_all, non_blocking=True)
        h_rec.copy_(d_rec, non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for k in range(nstreams):
            host_call(h_np[k], h_rnp[k], max_groups, cap)
        return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

    calls, times = measure([("dgroups", dgroups), ("records_only", records_only), ("packets", packets),
                            ("device_copy", lambda: d_dst.copy_(d_src))])
    host = [host_path() for _ in range(HOST_SAMPLES)]
    dgroups()
    torch.cuda.synchronize()
    ok = True
    for k in (0, nstreams - 1):
        ok = ok and d_dg[k].cpu().numpy().tobytes() == w_dg.tobytes() and d_sum[k].cpu().numpy().tobytes() == w_sm.tobytes()
        ok = ok and d_data[k].cpu().numpy().tobytes() == w_data.tobytes()
    if nframes <= 512:
        groups, summary = dgroups_model(one, rec0.view(PACKET_REC_DTYPE))
        got = np.frombuffer(w_dg.tobytes(), V.DGROUP_REC_DTYPE)
        ok = ok and summary["ngroups"] == int(sm["ngroups"]) and summary["n_dropped"] == int(sm["n_dropped"])
        ok = ok and all(bytes(w_data[r["offset"]:r["offset"] + r["length"]]) == g["D"] for g, r in zip(groups, got))
    med = {k: float(np.median(v)) for k, v in times.items()}
    d2h, loop = float(np.median([h[0] for h in host])), float(np.median([h[1] for h in host]))
    return {"logical_frames": nframes, "input": name, "streams": nstreams, "slots_per_stream": nslots, "groups_per_stream": int(sm["ngroups"]),
            "data_bytes_per_stream": cap, "packets_used": int(sm["n_used"]), "packets_dropped": int(sm["n_dropped"]),
            "bytes_read_plus_written": nstreams * moved, "calls_per_sample": calls,
            "ms": {k: round(v, 5) for k, v in med.items()},
            "ms_min_max": {k: [round(min(v), 5), round(max(v), 5)] for k, v in times.items()},
            "us_per_call": {k: round(1e3 * med[k] / nstreams, 2) for k in ("dgroups", "records_only", "packets")},
            "host_path_ms": {"d2h_copy": round(d2h, 4), "data_groups_host_loop": round(loop, 3), "total": round(d2h + loop, 3),
                             "total_min_max": [round(min(a + b for a, b in host), 3), round(max(a + b for a, b in host), 3)]},
            "dgroups_over_packets": round(med["dgroups"] / med["packets"], 2),
            "dgroups_over_device_copy": round(med["dgroups"] / med["device_copy"], 2),
            "host_path_over_dgroups": round((d2h + loop) / med["dgroups"], 2), "parity_ok": bool(ok)}


cases = []
for nf in (512, 4096):
    for name, p_lost in (("clean", 0.0), ("lost_2_percent", 0.02)):
        cases.append(run(nf, name, build_stream(nf, p_lost), NSTREAMS))
cases.append(run(4096, "worst_case_1021_addresses", worst_stream(4096), 1))
res = {"samples": samples, "min_sample_ms": MIN_MS, "host_samples": HOST_SAMPLES, "cases": cases}
line = json.dumps(res)
print(line)
if json_out:
    os.makedirs(os.path.dirname(os.path.abspath(json_out)), exist_ok=True)
    with open(json_out, "w") as f:
        f.write(line + "\n")
sys.exit(0 if all(c["parity_ok"] for c in res["cases"]) else 1)
