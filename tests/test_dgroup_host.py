"""CPU: MSC data groups from packets (include/viterbi_amd.h, "Packet mode": vit_data_groups_dev / vit_data_groups_host) -
a pure-Python model of the definition, the directed streams that visit every path of it (tests/test_gpu_dgroup.py imports
both), and the host twin against the model, byte for byte, behind guard patterns.

The model is the sequential walk per address - open at a first flag, break on a wrong continuity index or a new first
flag, close at a last flag - the form the kernels do not use (they join summaries of stretches of packets).  Its header
parser follows the header's text line by line and collects the bytes it names."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from test_packet_host import (PACKET_REC_DTYPE, PKT_CONT, PKT_DATA, PKT_FEC, PKT_OVERRUN, PKT_PADDING, SLOT,  # noqa: E402
                              crc16, fec_hdr, make_packet, packets_model)

PKT_LAST, PKT_FIRST = 4, 8
DGROUP_REC_DTYPE = np.dtype([("first_slot", "<u4"), ("last_slot", "<u4"), ("npackets", "<u4"), ("offset", "<u4"), ("length", "<u4"),
                             ("address", "<u2"), ("segment", "<u2"), ("transport_id", "<u2"), ("payload_offset", "<u2"),
                             ("type", "u1"), ("cont_rep", "u1"), ("flags", "u1"), ("command", "u1")])
DGROUP_SUM_DTYPE = np.dtype([("ngroups", "<u4"), ("nwritten", "<u4"), ("data_bytes", "<u4"), ("open_from", "<u4"), ("n_used", "<u4"),
                             ("n_dropped", "<u4"), ("n_unusable", "<u4"), ("reserved", "<u4")])
WELLFORMED, CRCF, CRC_OK, SEG, UA, TIDF, EXT = 1, 2, 4, 8, 16, 32, 64
GUARD = 0xA5
PAD_DG, PAD_SUM, PAD_DATA = 32, 16, 48   # guard bytes in front of the three outputs (and as many behind)


# ---- the model ------------------------------------------------------------------------------------------------------------
def usable(rec, i):
    r = rec[i]
    return r["kind"] == PKT_DATA and r["crc_ok"] == 1 and int(r["useful"]) <= 24 * int(r["nslots"]) - 5


def parse_header(D):
    """the record's header fields of a group's bytes D: a dict"""
    L = len(D)
    out = dict(type=0, cont_rep=0, flags=0, segment=0, transport_id=0, payload_offset=0)
    if L < 2:
        return out
    b0 = D[0]
    ext, crcf, seg, ua = b0 >> 7, (b0 >> 6) & 1, (b0 >> 5) & 1, (b0 >> 4) & 1
    out["type"], out["cont_rep"] = b0 & 15, D[1]
    end = L - (2 if crcf else 0)
    named = []          # the positions of the bytes the text names
    bad = False
    segment = tid = tidf = 0
    p = 2
    if ext:
        p += 2
    if seg:
        named += [p, p + 1]
        segment = (D[p] << 8 | D[p + 1]) if p + 1 < L else 0
        p += 2
    if ua:
        named.append(p)
        x = D[p] if p < L else 0
        li, tidf = x & 15, (x >> 4) & 1
        p += 1
        if tidf and li < 2:
            bad = True
        if tidf and li >= 2:
            named += [p, p + 1]
            tid = (D[p] << 8 | D[p + 1]) if p + 1 < L else 0
        p += li
    if bad or any(q >= end for q in named) or p > end:
        return out
    flags = WELLFORMED | crcf * CRCF | seg * SEG | ua * UA | tidf * TIDF | ext * EXT
    if crcf and crc16(D[:L - 2]) == (D[L - 2] << 8 | D[L - 1]):
        flags |= CRC_OK
    out.update(flags=flags, segment=segment, transport_id=tid, payload_offset=p)
    return out


def dgroups_model(stream, rec):
    """every data group of the window, in the order of their last slots, and the summary's counts: (groups, summary)
    with groups = dicts of first_slot, last_slot, npackets, address, command, D (bytes)"""
    stream = np.asarray(stream, np.uint8)
    n = len(rec)
    by_addr = {}
    unusable = 0
    for i in range(n):
        if usable(rec, i):
            by_addr.setdefault(int(rec["address"][i]), []).append(i)
        elif rec["kind"][i] == PKT_DATA:
            unusable += 1
    groups, dropped, open_from = [], 0, n
    for addr, slots in by_addr.items():
        cur = None      # the packets of the group being collected
        for i in slots:
            fl = int(rec["flags"][i])
            if fl & PKT_FIRST:
                dropped += len(cur) if cur else 0
                cur = [i]
            elif cur and (fl & 3) == ((int(rec["flags"][cur[-1]]) & 3) + 1) & 3:
                cur.append(i)
            else:
                dropped += (len(cur) if cur else 0) + 1
                cur = None
                continue
            if fl & PKT_LAST:
                D = b"".join(bytes(stream[SLOT * j + 3:SLOT * j + 3 + int(rec["useful"][j])]) for j in cur)
                groups.append(dict(first_slot=cur[0], last_slot=i, npackets=len(cur), address=addr, D=D,
                                   command=(int(rec["flags"][cur[0]]) >> 4) & 1))
                cur = None
        if cur:
            open_from = min(open_from, cur[0])
    groups.sort(key=lambda g: g["last_slot"])
    summary = dict(ngroups=len(groups), open_from=open_from, n_used=sum(g["npackets"] for g in groups), n_dropped=dropped,
                   n_unusable=unusable)
    return groups, summary


def expected_buffers(stream, rec, max_groups, capacity, with_data=True):
    """what a call leaves in guarded buffers: (dg bytes, summary bytes, data bytes or None), guards included"""
    groups, summary = dgroups_model(stream, rec)
    dg = np.full(PAD_DG + 32 * max_groups + PAD_DG, GUARD, np.uint8)
    data = np.full(PAD_DATA + capacity + PAD_DATA, GUARD, np.uint8) if with_data else None
    off = nwritten = 0
    for k, g in enumerate(groups):
        L = len(g["D"])
        if k == nwritten and k < max_groups and (not with_data or off + L <= capacity):
            r = np.zeros(1, DGROUP_REC_DTYPE)
            for f in ("first_slot", "last_slot", "npackets", "address", "command"):
                r[f] = g[f]
            r["offset"], r["length"] = off, L
            for f, v in parse_header(g["D"]).items():
                r[f] = v
            dg[PAD_DG + 32 * k:PAD_DG + 32 * (k + 1)] = np.frombuffer(r.tobytes(), np.uint8)
            if with_data:
                data[PAD_DATA + off:PAD_DATA + off + L] = np.frombuffer(g["D"], np.uint8)
            nwritten += 1
        off += (L + 15) // 16 * 16
    s = np.zeros(1, DGROUP_SUM_DTYPE)
    for f, v in summary.items():
        s[f] = v
    s["nwritten"], s["data_bytes"] = nwritten, off
    sm = np.full(PAD_SUM + 32 + PAD_SUM, GUARD, np.uint8)
    sm[PAD_SUM:PAD_SUM + 32] = np.frombuffer(s.tobytes(), np.uint8)
    return dg, sm, data


def total_bytes(stream, rec):
    return sum((len(g["D"]) + 15) // 16 * 16 for g in dgroups_model(stream, rec)[0])


# ---- builders -------------------------------------------------------------------------------------------------------------
def packet(rng, nslots, address, cont=0, first=0, last=0, command=0, useful=None, data=None):
    """make_packet with chosen data bytes"""
    if data is not None:
        useful = len(data)
    p = make_packet(rng, nslots, address, cont, first << 1 | last, command, useful)
    if data is not None and len(data):
        p[3:3 + len(data)] = np.frombuffer(bytes(data), np.uint8)
        c = crc16(p[:-2])
        p[-2], p[-1] = c >> 8, c & 255
    return p


def group_packets(rng, address, D, shape, cont0=0, command=0):
    """the packets of one group: shape = [(slots, useful), ...] with the usefuls summing to len(D)"""
    assert sum(u for _, u in shape) == len(D)
    out, at = [], 0
    for k, (n, u) in enumerate(shape):
        out.append(packet(rng, n, address, (cont0 + k) & 3, int(k == 0), int(k == len(shape) - 1), command, data=D[at:at + u]))
        at += u
    return out


def random_shape(rng, npackets):
    shape = []
    for _ in range(npackets):
        n = int(rng.integers(1, 5))
        shape.append((n, int(rng.integers(0, 24 * n - 5 + 1))))
    return shape


def random_group(rng, address, npackets, cont0=0):
    shape = random_shape(rng, npackets)
    D = bytes(rng.integers(0, 256, sum(u for _, u in shape), dtype=np.uint8))
    return group_packets(rng, address, D, shape, cont0)


def finish(parts, framebytes=None):
    st = np.concatenate(parts)
    return st, packets_model(st, framebytes or st.size)


def header_bytes(ext=0, crcf=0, seg=0, ua=0, tidf=0, li=0, payload=b"", typ=3, rng=None):
    """a group's bytes with the given header parts, a good CRC behind them if crcf"""
    rng = rng or np.random.default_rng(0)
    D = [ext << 7 | crcf << 6 | seg << 5 | ua << 4 | typ, int(rng.integers(0, 256))]
    if ext:
        D += [int(x) for x in rng.integers(0, 256, 2)]
    if seg:
        D += [int(x) for x in rng.integers(0, 256, 2)]
    if ua:
        D += [int(rng.integers(0, 8)) << 5 | tidf << 4 | li] + [int(x) for x in rng.integers(0, 256, li)]
    D = bytes(D) + bytes(payload)
    if crcf:
        c = crc16(D)
        D += bytes([c >> 8, c & 255])
    return D


def recrc(D):
    """D with its last two bytes set to the CRC of the bytes before them"""
    c = crc16(D[:-2])
    return D[:-2] + bytes([c >> 8, c & 255])


def two_packets(rng, address, D, cont0=0):
    """a group as two one- or two-slot packets, cut at a random byte (the header may straddle the cut)"""
    cut = int(rng.integers(0, len(D) + 1))
    cut = min(max(cut, len(D) - 43), 43)
    shape = [(1 if u <= 19 else 2, u) for u in (cut, len(D) - cut)]
    return group_packets(rng, address, D, shape, cont0)


def directed_streams():
    """name -> (stream, records): every path of the definition"""
    rng = np.random.default_rng(11)
    out = {}
    pk = lambda *a, **k: packet(rng, *a, **k)  # noqa: E731
    # run shapes
    out["one_packet"] = finish([pk(1, 5, 0, 1, 1, useful=9)])
    parts = []
    for npk, cont0 in ((2, 0), (3, 3), (5, 2), (9, 1)):     # the continuity index wraps in each of the longer ones
        parts += random_group(rng, 40, npk, cont0)
    out["groups_2_3_5_9"] = finish(parts)
    # breaks
    g = random_group(rng, 9, 4)
    out["break_wrong_cont"] = finish(g[:2] + [pk(1, 9, 3, 0, 0, useful=5)] + g[2:])
    out["break_skipped_packet"] = finish(g[:1] + g[2:])
    out["break_first_inside_then_succeeds"] = finish(g[:2] + random_group(rng, 9, 3, 2))
    out["packet_after_closed_run"] = finish(random_group(rng, 9, 2) + [pk(2, 9, 2, 0, 0), pk(1, 9, 3, 0, 1)] + random_group(rng, 9, 1))
    bad = g[1].copy()
    bad[5] ^= 0x10
    out["unusable_bad_crc_inside"] = finish([g[0], bad] + g[2:])
    out["unusable_useful_20_inside"] = finish([g[0], pk(1, 9, 1, 0, 0, useful=20)] + g[2:])
    out["replaced_by_unusable"] = finish([g[0], pk(1, 9, 1, 0, 0, useful=20), g[1]] + g[2:])   # the run goes on behind it
    # other slots between a group's packets
    fec = np.zeros(SLOT, np.uint8)
    fec[:2] = fec_hdr(4)
    fec[2:] = rng.integers(0, 256, 22, dtype=np.uint8)
    # frames of 4 slots: [g0 pad] [g1(<=2) ...] - an overrun: a 3-slot packet at slot 2 of a frame
    g1 = [packet(rng, 1, 300, k, int(k == 0), int(k == 3), useful=7 + k) for k in range(4)]
    over = pk(3, 300, 1, 0, 0)[:2 * SLOT]
    out["other_kinds_between"] = finish([g1[0], pk(2, 0), fec, g1[1], pk(3, 77, 0, 0, 0), g1[2], fec, over, g1[3], pk(1, 0), pk(2, 0)], 96)
    assert set(out["other_kinds_between"][1]["kind"].tolist()) == {PKT_CONT, PKT_DATA, PKT_PADDING, PKT_FEC, PKT_OVERRUN}
    ga, gb, gc = random_group(rng, 1, 5), random_group(rng, 1021, 5, 1), random_group(rng, 1023, 5, 2)
    out["three_addresses_interleaved"] = finish([p for t in zip(ga, gb, gc) for p in t])
    # window end
    g, h = random_group(rng, 12, 3), random_group(rng, 13, 4)
    out["open_run_at_end"] = finish(random_group(rng, 12, 2) + g[:2])
    out["two_open_runs"] = finish([pk(1, 99, 0, 1, 1)] + h[:1] + g[:1] + h[1:3] + g[1:2])
    out["no_open_run"] = finish(g + h + [pk(1, 12, 0, 0, 0)])
    out["open_head_without_first"] = finish(g[1:2] + h[:1])
    # sizes
    parts = []
    for n in (1, 2, 3, 4):
        parts += [pk(n, 20, 0, 1, 1, useful=0), pk(n, 20, 1, 1, 1, useful=24 * n - 5), pk(n, 20, 2, 1, 1, useful=min(24 * n - 4, 127))]
    parts += group_packets(rng, 21, b"\x07", [(1, 0), (2, 1), (1, 0)])          # length 1
    parts += group_packets(rng, 21, b"", [(1, 0), (1, 0)])                      # length 0
    parts += group_packets(rng, 21, bytes(rng.integers(0, 256, 91 * 3, dtype=np.uint8)), [(4, 91)] * 3)
    out["sizes"] = finish(parts)
    # headers: the 16 combinations, li 0 ... 15 where ua; each group cut into two packets somewhere
    parts, c = [], 0
    for ext in (0, 1):
        for seg in (0, 1):
            for ua in (0, 1):
                for tidf in (0, 1):
                    for li in (range(16) if ua else (0,)):
                        for crcf in ((0, 1) if li in (0, 2, 15) else (int(rng.integers(0, 2)),)):
                            D = header_bytes(ext, crcf, seg, ua, tidf, li, rng.integers(0, 256, int(rng.integers(0, 6)), dtype=np.uint8),
                                             int(rng.integers(0, 16)), rng)
                            parts += two_packets(rng, 7, D, c)
                            c += 2
    out["headers"] = finish(parts)
    # a header that ends exactly at the end, and one byte short, for each of its parts
    parts = []
    for kw in (dict(), dict(ext=1), dict(seg=1), dict(ext=1, seg=1), dict(ua=1, li=0), dict(ua=1, li=5), dict(ua=1, tidf=1, li=2),
               dict(ua=1, tidf=1, li=7), dict(ext=1, seg=1, ua=1, tidf=1, li=2), dict(seg=1, ua=1, li=1)):
        for crcf in (0, 1):
            D = header_bytes(crcf=crcf, rng=rng, **kw)
            short = recrc(D[:-3] + D[-2:]) if crcf else D[:-1]
            shorter = recrc(D[:-4] + D[-2:]) if crcf and len(D) >= 5 else short[:-1]     # (byte 0 stays)
            for d in (D, short, shorter, D + b"\x00" if not crcf else recrc(D[:-2] + b"\x00" + D[-2:])):
                parts += two_packets(rng, 8, d)
    out["header_edges"] = finish(parts)
    good = header_bytes(crcf=1, seg=1, payload=rng.integers(0, 256, 30, dtype=np.uint8), rng=rng)
    badcrc = good[:5] + bytes([good[5] ^ 1]) + good[6:]
    badlast = good[:-1] + bytes([good[-1] ^ 0x80])
    badfirst = good[:-2] + bytes([good[-2] ^ 1]) + good[-1:]
    out["crc_good_bad"] = finish(sum((group_packets(rng, 8, d, [(1, 19), (1, 0), (1, len(d) - 20), (1, 1)]) for d in
                                      (good, badcrc, badlast, badfirst)), []))
    return out


def random_stream(seed=5, ngroups=400, naddr=5, p_lost=0.05):
    """groups of 1 ... 8 packets at naddr addresses, interleaved, each packet lost with probability p_lost"""
    rng = np.random.default_rng(seed)
    addrs = [int(a) for a in rng.choice(np.arange(1, 1022), naddr, replace=False)]
    queues = {a: [] for a in addrs}
    cont = {a: 0 for a in addrs}
    for _ in range(ngroups):
        a = addrs[int(rng.integers(0, naddr))]
        g = random_group(rng, a, int(rng.integers(1, 9)), cont[a])
        cont[a] = (cont[a] + len(g)) & 3
        queues[a] += g
    parts = []
    while any(queues.values()):
        a = addrs[int(rng.integers(0, naddr))]
        if queues[a]:
            p = queues[a].pop(0)
            if rng.random() >= p_lost:
                parts.append(p)
    return finish(parts)


def synth_stream(rng, nslots, naddr=3, max_group=6, addrs=None):
    """a long stream without real packet CRCs (the records say crc_ok): random packets of groups at naddr addresses,
    interleaved, some padding; the records are written directly, as vit_packets_dev would for good packets"""
    st = rng.integers(0, 256, SLOT * nslots, dtype=np.uint8)
    rec = np.zeros(nslots, PACKET_REC_DTYPE)
    addrs = addrs or [int(a) for a in rng.choice(np.arange(1, 1022), naddr, replace=False)]
    state = {a: [0, 0] for a in addrs}   # packets left in the group, continuity index
    i = 0
    while i < nslots:
        n = min(int(rng.integers(1, 5)), nslots - i)
        a = addrs[int(rng.integers(0, len(addrs)))] if rng.random() < 0.9 else 0
        useful = int(rng.integers(0, 24 * n - 5 + 1))
        first = last = 0
        if a:
            left, c = state[a]
            if left == 0:
                left, first = int(rng.integers(1, max_group + 1)), 1
            left -= 1
            last = int(left == 0)
            if rng.random() < 0.03:
                c = (c + 1) & 3      # a lost packet
            state[a] = [left, (c + 1) & 3]
            cont = c
        else:
            cont = 0
        st[SLOT * i] = (n - 1) << 6 | cont << 4 | first << 3 | last << 2 | a >> 8
        st[SLOT * i + 1] = a & 255
        st[SLOT * i + 2] = useful
        rec[i] = (PKT_DATA if a else PKT_PADDING, 1, n, cont | last << 2 | first << 3, a, useful, 0)
        i += n
    return st, rec


# ---- the host twin ----------------------------------------------------------------------------------------------------------
def call_host(V, stream, rec, max_groups, capacity, with_data=True):
    dg = np.full(PAD_DG + 32 * max_groups + PAD_DG, GUARD, np.uint8)
    sm = np.full(PAD_SUM + 32 + PAD_SUM, GUARD, np.uint8)
    data = np.full(PAD_DATA + capacity + PAD_DATA, GUARD, np.uint8) if with_data else None
    stream, rec = np.ascontiguousarray(stream, np.uint8), np.ascontiguousarray(rec)
    rc = V.lib().vit_data_groups_host(stream.ctypes.data, rec.ctypes.data, len(rec), dg.ctypes.data + PAD_DG, max_groups,
                                      sm.ctypes.data + PAD_SUM, data.ctypes.data + PAD_DATA if with_data else None, capacity)
    assert rc == 0, V.last_error()
    return dg, sm, data


def same_buffers(got, want, what):
    for name, g, w in zip(("records", "summary", "data"), got, want):
        if w is None:
            assert g is None
            continue
        assert g.shape == w.shape
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, "%s: %s differ at byte %d (of %d): got %s, want %s" % (
            what, name, bad[0], g.size, g[bad[0]:bad[0] + 8].tolist(), w[bad[0]:bad[0] + 8].tolist())


DIRECTED = directed_streams()


def test_model_on_the_directed_streams():
    """the streams do what their names say (the model alone)"""
    def run(name):
        g, s = dgroups_model(*DIRECTED[name])
        return g, s, len(DIRECTED[name][1])
    g, s, n = run("one_packet")
    assert len(g) == 1 and g[0]["npackets"] == 1 and s["n_dropped"] == 0 and s["open_from"] == n
    g, s, n = run("groups_2_3_5_9")
    assert [x["npackets"] for x in g] == [2, 3, 5, 9] and s["n_used"] == 19
    assert run("break_wrong_cont")[1]["n_dropped"] == 5 and run("break_wrong_cont")[1]["ngroups"] == 0
    assert run("break_skipped_packet")[1]["n_dropped"] == 3
    g, s, n = run("break_first_inside_then_succeeds")
    assert len(g) == 1 and g[0]["npackets"] == 3 and s["n_dropped"] == 2
    g, s, n = run("packet_after_closed_run")
    assert [x["npackets"] for x in g] == [2, 1] and s["n_dropped"] == 2
    for name in ("unusable_bad_crc_inside", "unusable_useful_20_inside"):
        g, s, n = run(name)
        assert len(g) == 0 and s["n_unusable"] == 1 and s["n_dropped"] == 3
    g, s, n = run("replaced_by_unusable")
    assert len(g) == 1 and g[0]["npackets"] == 4 and s["n_unusable"] == 1
    g, s, n = run("other_kinds_between")
    assert len(g) == 1 and g[0]["npackets"] == 4 and len(g[0]["D"]) == 7 + 8 + 9 + 10
    g, s, n = run("three_addresses_interleaved")
    assert [x["address"] for x in g] == [1, 1021, 1023] and [x["last_slot"] for x in g] == sorted(x["last_slot"] for x in g)
    g, s, n = run("open_run_at_end")
    assert len(g) == 1 and s["open_from"] == g[0]["last_slot"] + int(DIRECTED["open_run_at_end"][1]["nslots"][g[0]["last_slot"]])
    g, s, n = run("two_open_runs")
    assert s["open_from"] == 1 and s["n_dropped"] == 0 and s["n_used"] == 1
    assert run("no_open_run")[1]["open_from"] == run("no_open_run")[2] and run("no_open_run")[1]["n_dropped"] == 1
    g, s, n = run("open_head_without_first")
    assert s["open_from"] == int(DIRECTED["open_head_without_first"][1]["nslots"][0]) and s["n_dropped"] == 1
    g, s, n = run("sizes")
    assert sorted(set(len(x["D"]) for x in g)) == [0, 1, 19, 43, 67, 91, 273] and s["n_unusable"] == 4
    hs = [parse_header(x["D"]) for x in run("headers")[0]]
    assert {h["flags"] & (EXT | SEG | UA | TIDF) for h in hs if h["flags"]} == {e | s_ | u for e in (0, EXT) for s_ in (0, SEG)
                                                                             for u in (0, UA, UA | TIDF)}
    assert sum(1 for h in hs if not h["flags"]) == 4 * 3    # tidf with li 0 (with and without a CRC) and li 1, per ext and seg
    hs = [parse_header(x["D"]) for x in run("header_edges")[0]]
    assert [bool(h["flags"]) for h in hs][:4] == [True, False, False, True] and sum(1 for h in hs if h["flags"]) == 40
    hs = [parse_header(x["D"]) for x in run("crc_good_bad")[0]]
    assert [h["flags"] & CRC_OK for h in hs] == [CRC_OK, 0, 0, 0] and all(h["flags"] & WELLFORMED for h in hs)


@pytest.mark.parametrize("name", sorted(DIRECTED))
def test_host_twin_directed(V, name):
    stream, rec = DIRECTED[name]
    cap = total_bytes(stream, rec)
    ng = dgroups_model(stream, rec)[1]["ngroups"]
    same_buffers(call_host(V, stream, rec, ng + 2, cap + 5), expected_buffers(stream, rec, ng + 2, cap + 5), name)
    same_buffers(call_host(V, stream, rec, ng + 2, 0, False), expected_buffers(stream, rec, ng + 2, 0, False), name + " records only")


def capacity_cases(stream, rec):
    """(max_groups, capacity, with_data) at the edges"""
    groups = dgroups_model(stream, rec)[0]
    ng, total = len(groups), total_bytes(stream, rec)
    exact = total - (len(groups[-1]["D"]) + 15) // 16 * 16 + len(groups[-1]["D"])
    assert ng >= 3 and len(groups[-1]["D"]) > 0
    return [(0, total, True), (ng - 1, total, True), (ng, total, True), (ng, exact - 1, True), (ng, exact, True), (ng, 0, True),
            (ng, 0, False), (1, 0, False), (0, 0, False)]


def test_host_twin_capacity(V):
    stream, rec = DIRECTED["groups_2_3_5_9"]
    for mg, cap, wd in capacity_cases(stream, rec):
        same_buffers(call_host(V, stream, rec, mg, cap, wd), expected_buffers(stream, rec, mg, cap, wd), "max_groups %d capacity %d" % (mg, cap))
    # a group of length 0 in front fits into no room at all
    stream, rec = finish([packet(np.random.default_rng(1), 1, 5, 0, 1, 1, useful=0)] + list(np.split(stream, len(stream) // SLOT)))
    got = call_host(V, stream, rec, 4, 0)
    same_buffers(got, expected_buffers(stream, rec, 4, 0), "capacity 0")
    assert np.frombuffer(got[1][PAD_SUM:PAD_SUM + 32].tobytes(), DGROUP_SUM_DTYPE)["nwritten"][0] == 1


def test_host_twin_argument_errors(V):
    L = V.lib()
    stream, rec = DIRECTED["one_packet"]
    dg, sm, data = np.zeros(64, np.uint8), np.zeros(32, np.uint8), np.zeros(64, np.uint8)
    s, r, d, m, x = stream.ctypes.data, rec.ctypes.data, dg.ctypes.data, sm.ctypes.data, data.ctypes.data
    assert L.vit_data_groups_host(s, r, 1, d, 2, m, x, 64) == 0
    for args in ((None, r, 1, d, 2, m, x, 64), (s, None, 1, d, 2, m, x, 64), (s, r, 1, d, 2, None, x, 64), (s, r, 1, None, 2, m, x, 64),
                 (s, r, -1, d, 2, m, x, 64), (s, r, (1 << 24) + 1, d, 2, m, x, 64), (s, r, 1, d, 2, m, None, 64)):
        assert L.vit_data_groups_host(*args) == 1 and "vit_data_groups_host" in V.last_error()
    assert L.vit_data_groups_host(s, r, 1, None, 0, m, None, 0) == 0      # records-only with no room: the summary alone
    sm[:] = GUARD
    assert L.vit_data_groups_host(None, None, 0, None, 0, None, None, 0) == 0 and L.vit_data_groups_host(s, r, 0, d, 2, m, x, 64) == 0
    assert (sm == GUARD).all()


def test_binding(V):
    assert V.DGROUP_REC_DTYPE == DGROUP_REC_DTYPE and V.DGROUP_SUM_DTYPE == DGROUP_SUM_DTYPE
    assert DGROUP_REC_DTYPE.itemsize == 32 and DGROUP_SUM_DTYPE.itemsize == 32 and (V.PKT_FIRST, V.PKT_LAST) == (PKT_FIRST, PKT_LAST)
    assert all(isinstance(v, int) and v > 0 for v in V.DGROUP_GEOMETRY.values()) and len(V.DGROUP_GEOMETRY) >= 3
    stream, rec = DIRECTED["groups_2_3_5_9"]
    groups, summary = dgroups_model(stream, rec)
    dg, sm, data = V.data_groups_host(stream, rec, 8, 4096)
    assert len(dg) == 4 and sm["ngroups"] == 4 and sm["n_used"] == 19 and data.size == 4096
    for g, r in zip(groups, dg):
        assert bytes(data[r["offset"]:r["offset"] + r["length"]]) == g["D"] and r["address"] == 40
    dg, sm, data = V.data_groups_host(stream, rec, 2, None)
    assert len(dg) == 2 and data is None and sm["nwritten"] == 2


def test_host_twin_random_stream(V):
    stream, rec = random_stream()
    groups, summary = dgroups_model(stream, rec)
    assert len(groups) >= 200 and summary["n_dropped"] >= 50, "vacuous: %d groups, %d dropped" % (len(groups), summary["n_dropped"])
    cap = total_bytes(stream, rec)
    same_buffers(call_host(V, stream, rec, len(groups), cap), expected_buffers(stream, rec, len(groups), cap), "random stream")


def test_host_twin_synthetic_stream(V):
    """the builder of the long streams of tests/test_gpu_dgroup.py: its records are what vit_packets_dev writes for good packets"""
    rng = np.random.default_rng(9)
    stream, rec = synth_stream(rng, 700)
    want = packets_model(stream, stream.size)
    assert (rec["kind"] == want["kind"]).all() and (rec["flags"] == want["flags"]).all() and (rec["address"] == want["address"]).all()
    assert (rec["useful"] == want["useful"]).all() and (rec["nslots"] == want["nslots"]).all()
    groups, summary = dgroups_model(stream, rec)
    assert len(groups) >= 40 and summary["n_dropped"] >= 5
    cap = total_bytes(stream, rec)
    same_buffers(call_host(V, stream, rec, len(groups), cap), expected_buffers(stream, rec, len(groups), cap), "synthetic stream")
