#!/usr/bin/env python3
"""A whole ensemble per call: vit_ensemble_dev against the loop a caller wrote before it (vit_dabplus_ti_superframes_dev +
vit_dabplus_aus_dev per sub-channel on one stream), and vit_rs_table_dev + vit_dabplus_aus_table_dev against the 36
uniform launches they replace.

Workload: a mode-I ensemble (864 CUs, 55296 columns per CIF) of 18 DAB+ sub-channels, RSDims 4 x 12, 6 x 8, 6 x 6, 2 x 4
(138 of the 144 a rate-1/2 ensemble can hold), each under a rate-1/2 profile (symbols 0 and 1 of every step), superframes
starting at CIF phases 0 ... 4, at nsf = 16 (80 CIFs) and nsf = 512 superframes per sub-channel.  Every sub-channel repeats
two distinct superframes sent through an AWGN channel at Eb/N0 = 2.5 dB for the punctured rate, where the decoder leaves RS
a few columns to correct in most superframes (counted in the result, and checked against the oracle).

HIP-event times through the C ABI with the arguments prepared once (no Python between the calls of a variant but the
ctypes call itself); the variants of a comparison alternate; every sample repeats its variant until it lasts 0.1 s;
median of the samples, min and max for the spread.  Parity: all five output buffers of the chain equal the loop's.

usage: bench_ensemble.py [samples]"""
import ctypes as C
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
from test_dab_host import scramble  # noqa: E402
from test_gpu_dab import dabplus_superframes  # noqa: E402
from test_punct_host import depuncture, puncture  # noqa: E402
from test_ti_host import CU, periodic_cif  # noqa: E402

V = _vitpkg.load_package()
O = _vitpkg.load_oracle()
O.build()
assert V.initialize() and V.device_count() >= 1, V.last_error()
V.set_renorm_ge(0)
L = V.lib()
samples = int(sys.argv[1]) if len(sys.argv) > 1 else 9
MIN_SAMPLE_MS = 100.0
RSDIMS = [12] * 4 + [8] * 6 + [6] * 6 + [4] * 2
ROW = 864 * CU
REC = 20
rng = np.random.default_rng(2030)


def timed(fn, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / k


def alternate(fns, warm=3):
    """per fn: (median ms, samples, repeats per sample); the fns alternating"""
    for _ in range(warm):  # code objects, scratch growth
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    reps = [max(1, int(np.ceil(MIN_SAMPLE_MS / timed(fn, 3)))) for fn in fns]
    ts = [[] for _ in fns]
    for _ in range(samples):
        for t, fn, k in zip(ts, fns, reps):
            t.append(timed(fn, k))
    return [(float(np.median(t)), t, k) for t, k in zip(ts, reps)]


def stat(res):
    ms, t, k = res
    return {"ms": round(ms, 4), "ms_min_max": [round(min(t), 4), round(max(t), 4)], "spread": round((max(t) - min(t)) / ms, 4),
            "calls_per_sample": k}


def compare(base, new):
    """new against base: the ratio of the medians, and whether new wins by more than the two spreads together"""
    a, b = stat(base), stat(new)
    ratio = b["ms"] / a["ms"]
    return {"ratio": round(ratio, 4), "wins_by_more_than_both_spreads": bool(1.0 - ratio > a["spread"] + b["spread"])}


def soft_symbols(sf, r, ebn0_db=2.5, rate=0.5):
    """superframes -> 5 scrambled frames each -> the mother code's symbols, soft, AWGN at Eb/N0 for the punctured rate"""
    fb = 192 * r
    frames = scramble(sf.reshape(-1, 24 * r), fb)
    hard = np.stack([O.encode(b) for b in np.unpackbits(frames, axis=1)[:, :fb]]).astype(np.float64)
    sigma = np.sqrt(1.0 / (2 * rate * 10 ** (ebn0_db / 10)))
    y = (2 * hard - 1) + sigma * rng.standard_normal(hard.shape)
    return np.clip(np.round(127.5 + 50 * y), 0, 255).astype(np.uint8)


# ---- the ensemble: two superframes per sub-channel, periodic ------------------------------------------------------------
oracle_ret = []  # per sub-channel: the oracle's RS return values of its two superframes
subs, pos = [], 0  # (rsdims, segs, start CU, phase, punctured base frames (10, P) rolled to the phase)
for k, r in enumerate(RSDIMS):
    fb = 192 * r
    segs = [(fb, 0x33333333), (6, 0x333333)]
    _, sf = dabplus_superframes(rng, 2, r)
    punct = puncture(soft_symbols(sf, r), segs, fb)
    phase = k % 5
    work = scramble(O.decode_batch(fb, depuncture(punct, segs, fb, 128), nthreads=16), fb).reshape(2, -1)
    oracle_ret.append(O.rs_check_batch(work, r, np.zeros((2, 110 * r), np.uint8))[0])
    subs.append((r, segs, pos, phase, np.roll(punct, phase, axis=0)))  # call frame phase + j = the stream's frame j
    pos += (punct.shape[1] + CU - 1) // CU
assert pos <= 864, pos
d_prof = torch.from_numpy(V.profiles_bytes([s[1] for s in subs])).cuda()
profiles = [V.punct_profile(s[1]) for s in subs]
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731

result = {"workload": {"rsdims": RSDIMS, "row_bytes": ROW, "cus_used": pos, "profile": "symbols 0 and 1 of every step"},
          "samples": samples, "min_sample_ms": MIN_SAMPLE_MS}
ok = True
for nsf in (16, 512):
    nrows = 5 * nsf + 4 + 15
    base = np.zeros((10, ROW), np.uint8)
    for r, segs, start, phase, punct in subs:
        base[:, CU * start:CU * start + punct.shape[1]] = punct
    d_ring = torch.from_numpy(periodic_cif(base, 10)).cuda().repeat((nrows + 9) // 10, 1)[:nrows].contiguous()
    sub = np.zeros(len(subs), V.ENS_SUBCH_DTYPE)
    for k, (r, segs, start, phase, punct) in enumerate(subs):
        sub[k] = (CU * start, k, 192 * r, r, phase, 5 * nsf, punct.shape[1], 0)
    lay = V.ensemble_layout(sub)
    assert int(lay["rows_needed"]) == nrows
    nrec = int(lay["nrec"])

    def outputs():
        return [torch.full((int(lay["work_bytes"]),), 0xEE, dtype=torch.uint8, device="cuda"),
                torch.full((int(lay["rs_bytes"]),), 0xA5, dtype=torch.uint8, device="cuda"),
                torch.full((nrec,), 0x7777, dtype=torch.int32, device="cuda"),
                torch.full((nrec,), 0xEE, dtype=torch.uint8, device="cuda"),
                torch.full((nrec * REC,), 0xEE, dtype=torch.uint8, device="cuda")]

    a, b, c = outputs(), outputs(), outputs()
    ring = V.cif_ring(d_ring, 0)
    rings = []
    for k in range(len(subs)):
        rk = V.cif_ring(d_ring, int(sub[k]["phase"]))
        rings.append(rk)
    loop_args, tail_args = [], []
    for k, (r, segs, start, phase, punct) in enumerate(subs):
        wo, ro, ri = (int(lay[n][k]) for n in ("work_offset", "rs_offset", "rec_index"))
        loop_args.append(((C.byref(rings[k]), CU * start, C.byref(profiles[k]), 128, ptr(a[0], wo), ptr(a[1], ro), ptr(a[2], 4 * ri),
                           ptr(a[3], ri), r, nsf, stream),
                          (ptr(a[1], ro), 110 * r, r, nsf, ptr(a[2], 4 * ri), ptr(a[4], REC * ri), stream)))
        tail_args.append(((ptr(a[0], wo), ptr(c[1], ro), ptr(c[2], 4 * ri), r, nsf, stream),
                          (ptr(c[1], ro), 110 * r, r, nsf, ptr(c[2], 4 * ri), ptr(c[4], REC * ri), stream)))
    sub_p = sub.ctypes.data_as(C.c_void_p)
    chain_args = (C.byref(ring), 0, sub_p, len(subs), ptr(d_prof), len(subs), 128, ptr(b[0]), ptr(b[1]), ptr(b[2]), ptr(b[3]),
                  ptr(b[4]), stream)

    def loop():
        for chain, aus in loop_args:
            assert L.vit_dabplus_ti_superframes_dev(*chain) == 0 and L.vit_dabplus_aus_dev(*aus) == 0

    def chain():
        assert L.vit_ensemble_dev(*chain_args) == 0, V.last_error()

    def uniform_tail():  # RS and access units on the loop's d_work: 36 launches
        for rs, aus in tail_args:
            assert L.vit_rs_batch_dev(*rs) == 0 and L.vit_dabplus_aus_dev(*aus) == 0

    def table_tail():  # the same on the chain's d_work: 2 launches
        assert L.vit_rs_table_dev(ptr(b[0]), ptr(b[1]), ptr(b[2]), sub_p, len(subs), stream) == 0
        assert L.vit_dabplus_aus_table_dev(ptr(b[1]), 0, sub_p, len(subs), ptr(b[2]), ptr(b[4]), stream) == 0

    whole = alternate([loop, chain])
    parity = all(bool((x == y).all()) for x, y in zip(a, b))
    tails = alternate([uniform_tail, table_tail])
    parity_tail = all(bool((b[i] == a[i]).all()) and bool((c[i] == a[i]).all()) for i in (1, 2, 4))
    rets = a[2].cpu().numpy()
    parity_oracle = np.array_equal(rets.reshape(len(subs), nsf // 2, 2), np.stack(oracle_ret)[:, None, :].repeat(nsf // 2, axis=1))
    ok = ok and parity and parity_tail and parity_oracle
    result["nsf_%d" % nsf] = {
        "frames": int(len(subs) * 5 * nsf), "superframes": nrec, "ring_rows": nrows,
        "superframes_corrected": int((rets > 0).sum()), "superframes_failed": int((rets < 0).sum()),
        "loop_36_calls": stat(whole[0]), "ensemble_dev": stat(whole[1]), "ensemble_vs_loop": compare(whole[0], whole[1]),
        "uniform_rs_aus_36_launches": stat(tails[0]), "table_rs_aus_2_launches": stat(tails[1]),
        "table_vs_uniform": compare(tails[0], tails[1]), "parity_ok": bool(parity), "parity_tail_ok": bool(parity_tail),
        "rs_returns_equal_the_oracle": bool(parity_oracle)}
    del d_ring, a, b, c

print(json.dumps(result))
sys.exit(0 if ok else 1)
