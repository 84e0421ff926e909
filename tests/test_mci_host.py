"""CPU: the multiplex configuration (include/viterbi_amd.h, "Multiplex configuration") - a pure-Python model of the FIB
walk and of last-wins per group that names every path it takes, the builders of FIGs and FIBs (tests/test_gpu_mci.py
imports both), vit_mci_fibs_host against the model in every byte, and the two host-only steps behind it: vit_eep_profile
and vit_mci_ens_table.

The model goes forward through a group's entries and compares each with the last one; the library's host twin goes
backward, the kernel by keys and atomics.  The constants of the format stand once, below."""
import ctypes as C
import os
import sys
from collections import Counter

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from test_dab_host import make_fib  # noqa: E402

# ---- the format (the library's: csrc/vit_fig_fmt.h) ---------------------------------------------------------------------
MCI_SUBCH_DTYPE = np.dtype([("org", "<u4"), ("comp", "<u4"), ("sid", "<u4"), ("n_org", "<u2"), ("n_org_other", "<u2"),
                            ("n_comp", "<u2"), ("n_comp_other", "<u2")])
MCI_GROUP_DTYPE = np.dtype([("eid", "<u2"), ("cif", "<u2"), ("flags", "u1"), ("reserved", "u1"), ("nfib_used", "<u2"),
                            ("nfib_malformed", "<u2"), ("n_ens_other", "<u2"), ("n_next", "<u2"), ("reserved2", "<u2")])
ST_USED, ST_MALFORMED, ST_FIG00, ST_FIG01, ST_FIG02 = 1, 2, 4, 8, 16
PRESENT, LONG = 1 << 31, 1 << 30
MAX_G = 4096

# every path of the model; the tests below must visit them all
LABELS = frozenset("""fib_unused fib_used end_marker_at_0 end_marker ran_to_30 overrun len0 type_1_to_7
ext_other cn_set oe_set fig00_4 fig00_5 fig00_short fig0_no_entries fig01_short fig01_long fig01_cut_below_3 fig01_long_cut
fig02_sid16 fig02_sid32 fig02_header_cut fig02_comp_cut fig02_nc0 tmid0 tmid1 tmid2 tmid3
org_first org_equal org_other comp_first comp_equal comp_other ens_first ens_same ens_other group_without_fig00""".split())


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the model --------------------------------------------------------------------------------------------------------
def walk_model(b, paths):
    """one used FIB (30 bytes at least) -> (status, n_next, entries); an entry is ('org', SubChId, org), ('comp', SubChId,
    (comp, sid)) or ('ens', 0, (eid, change, al, cif))"""
    b = [int(x) for x in b[:30]]
    st, n_next, out, p = ST_USED, 0, [], 0
    while True:
        if p >= 30:
            paths["ran_to_30"] += 1
            break
        h = b[p]
        if h == 0xFF:
            paths["end_marker_at_0" if p == 0 else "end_marker"] += 1
            break
        typ, ln = h >> 5, h & 31
        if p + 1 + ln > 30:
            paths["overrun"] += 1
            st |= ST_MALFORMED
            break
        if ln == 0:
            paths["len0"] += 1
        elif typ != 0:
            paths["type_1_to_7"] += 1
        else:
            t = b[p + 1]
            ext, q, e = t & 31, p + 2, p + 1 + ln
            if ext > 2:
                paths["ext_other"] += 1
            elif t & 0xC0:
                if t & 0x80:
                    paths["cn_set"] += 1
                if t & 0x40:
                    paths["oe_set"] += 1
                n_next += 1
            elif ext == 0:
                st |= ST_FIG00
                if e - q < 4:
                    paths["fig00_short"] += 1
                    st |= ST_MALFORMED
                else:
                    paths["fig00_4" if e - q == 4 else "fig00_5"] += 1
                    out.append(("ens", 0, (b[q] << 8 | b[q + 1], b[q + 2] >> 6, (b[q + 2] >> 5) & 1, (b[q + 2] & 31) << 8 | b[q + 3])))
            elif ext == 1:
                st |= ST_FIG01
                if q == e:
                    paths["fig0_no_entries"] += 1
                while q < e:
                    if e - q < 3:
                        paths["fig01_cut_below_3"] += 1
                        st |= ST_MALFORMED
                        break
                    sub, start = b[q] >> 2, (b[q] & 3) << 8 | b[q + 1]
                    if b[q + 2] >> 7 == 0:
                        paths["fig01_short"] += 1
                        out.append(("org", sub, PRESENT | start | (b[q + 2] & 63) << 10 | ((b[q + 2] >> 6) & 1) << 16))
                        q += 3
                    elif e - q < 4:
                        paths["fig01_long_cut"] += 1
                        st |= ST_MALFORMED
                        break
                    else:
                        paths["fig01_long"] += 1
                        size = (b[q + 2] & 3) << 8 | b[q + 3]
                        out.append(("org", sub, PRESENT | LONG | start | size << 10 | ((b[q + 2] >> 2) & 3) << 20 |
                                    ((b[q + 2] >> 4) & 7) << 22))
                        q += 4
            else:
                st |= ST_FIG02
                pd = (t >> 5) & 1
                if q == e:
                    paths["fig0_no_entries"] += 1
                leave = False
                while q < e and not leave:
                    nsid = 4 if pd else 2
                    if e - q < nsid + 1:
                        paths["fig02_header_cut"] += 1
                        st |= ST_MALFORMED
                        break
                    paths["fig02_sid32" if pd else "fig02_sid16"] += 1
                    sid = int.from_bytes(bytes(b[q:q + nsid]), "big")
                    nc = b[q + nsid] & 15
                    q += nsid + 1
                    if nc == 0:
                        paths["fig02_nc0"] += 1
                    for _ in range(nc):
                        if e - q < 2:
                            paths["fig02_comp_cut"] += 1
                            st |= ST_MALFORMED
                            leave = True
                            break
                        c0, c1 = b[q], b[q + 1]
                        tmid = c0 >> 6
                        paths["tmid%d" % tmid] += 1
                        if tmid <= 1:
                            out.append(("comp", c1 >> 2, (PRESENT | tmid | (c0 & 63) << 2 | ((c1 >> 1) & 1) << 8 | (c1 & 1) << 9, sid)))
                        q += 2
        p += 1 + ln
    return st, n_next, out


def mci_model(fibs, ok, G, paths=None, memo=None):
    """-> (MCI_SUBCH_DTYPE (ngroups, 64), MCI_GROUP_DTYPE (ngroups,), status bytes) by the definition of the header.
    memo: a dict that keeps the walk of every distinct FIB (its paths are then counted once)"""
    paths = Counter() if paths is None else paths
    fibs = np.asarray(fibs, np.uint8).reshape(-1, 32)
    n = fibs.shape[0]
    ng = (n + G - 1) // G
    sub, grp, status = np.zeros((ng, 64), MCI_SUBCH_DTYPE), np.zeros(ng, MCI_GROUP_DTYPE), np.zeros(n, np.uint8)
    for g in range(ng):
        ents, used, malf, nxt = [], 0, 0, 0
        for f in range(g * G, min((g + 1) * G, n)):
            if ok is not None and not ok[f]:
                paths["fib_unused"] += 1
                continue
            paths["fib_used"] += 1
            if memo is None:
                st, k, e = walk_model(fibs[f], paths)
            else:
                key = fibs[f, :30].tobytes()
                if key not in memo:
                    memo[key] = walk_model(fibs[f], paths)
                st, k, e = memo[key]
            status[f] = st
            used += 1
            malf += bool(st & ST_MALFORMED)
            nxt += k
            ents += e
        last = {}
        for kind, c, v in ents:
            last[(kind, c)] = v
        met = set()
        for kind, c, v in ents:
            r = sub[g, c]
            w = last[(kind, c)]
            differs = v[:3] != w[:3] if kind == "ens" else v != w   # (the CIF counter of a FIG 0/0 is not compared)
            if (kind, c) not in met:
                paths[kind + "_first"] += 1
            else:
                paths[kind + ("_other" if differs else "_same" if kind == "ens" else "_equal")] += 1
            met.add((kind, c))
            if kind == "org":
                r["org"] = w
                r["n_org" if v == w else "n_org_other"] += 1
            elif kind == "comp":
                r["comp"], r["sid"] = w
                r["n_comp" if v == w else "n_comp_other"] += 1
            else:
                grp[g]["eid"], grp[g]["cif"] = w[0], w[3]
                grp[g]["flags"] = 1 | w[1] << 1 | w[2] << 3
                grp[g]["n_ens_other"] += v[:3] != w[:3]
        if ("ens", 0) not in last:
            paths["group_without_fig00"] += 1
        grp[g]["nfib_used"], grp[g]["nfib_malformed"], grp[g]["n_next"] = used, malf, nxt
    return sub, grp, status


# ---- builders ---------------------------------------------------------------------------------------------------------
def fig(typ, body):
    assert len(body) <= 31
    return bytes([typ << 5 | len(body)]) + bytes(body)


def fig0(ext, cn, oe, pd, body):
    return fig(0, bytes([cn << 7 | oe << 6 | pd << 5 | ext]) + bytes(body))


def fig00(eid, change, al, cif, extra=b""):
    return fig0(0, 0, 0, 0, bytes([eid >> 8, eid & 255, change << 6 | al << 5 | cif >> 8, cif & 255]) + bytes(extra))


def fig01_short(sub, start, switch, index):
    return bytes([sub << 2 | start >> 8, start & 255, switch << 6 | index])


def fig01_long(sub, start, option, level, size):
    return bytes([sub << 2 | start >> 8, start & 255, 0x80 | option << 4 | level << 2 | size >> 8, size & 255])


def comp(tmid, typ, sub, ps=1, ca=0):
    return bytes([tmid << 6 | typ, sub << 2 | ps << 1 | ca])


def fig02_service(sid, comps, pd=0, nc=None, top=0):
    """the service header and its components; nc: the count byte's low bits if they are to differ from len(comps)"""
    return sid.to_bytes(4 if pd else 2, "big") + bytes([top << 4 | (len(comps) if nc is None else nc)]) + b"".join(comps)


def fill(*figs):
    """FIGs -> 30 bytes, padded with the end marker and zeros"""
    b = b"".join(figs)
    assert len(b) <= 30
    if len(b) < 30:
        b += b"\xff" + bytes(29 - len(b))
    return np.frombuffer(b, np.uint8)


def fib(*figs):
    return make_fib(fill(*figs))


def raw_fib(payload):
    p = np.zeros(30, np.uint8)
    p[:len(payload)] = np.frombuffer(bytes(payload), np.uint8)
    return make_fib(p)


def directed():
    """name -> (FIBs (k, 32), their flags or None): one case per path of the walk and of last-wins"""
    L1 = fig01_long(5, 100, 0, 2, 48)
    L2 = fig01_long(5, 100, 0, 2, 54)
    S1 = fig02_service(0x1234, [comp(0, 63, 5)])
    c = {}
    c["end marker at byte 0"] = [raw_fib(b"\xff" + fig0(1, 0, 0, 0, L1))]
    full = [fig0(1, 0, 0, 0, L1 + fig01_short(6, 10, 0, 3) * 2), fig0(2, 0, 0, 0, S1), fig00(0xABCD, 0, 0, 1), fig(1, bytes(4))]
    assert len(b"".join(full)) == 30
    c["30 bytes, no marker"] = [fib(*full)]
    c["length overrun by 1"] = [raw_fib(fig0(1, 0, 0, 0, L1) + bytes([0 << 5 | 24, 1]) + bytes(22))]
    c["len == 0 headers"] = [raw_fib(bytes([0x00, 0x20, 0xE0]) + fig0(1, 0, 0, 0, L1) + b"\x00\xff")]
    c["types 1 ... 7"] = [fib(*[fig(t, bytes([0x01, 0x14])) for t in range(1, 8)], fig0(1, 0, 0, 0, L1))]
    c["other extensions"] = [fib(fig0(3, 0, 0, 0, L1), fig0(31, 0, 0, 0, L1), fig0(13, 0, 0, 1, S1), fig0(1, 0, 0, 0, L2))]
    c["C/N and OE"] = [fib(fig0(1, 1, 0, 0, L2), fig0(2, 0, 1, 0, S1), fig0(0, 1, 1, 0, bytes(4)), fig0(1, 0, 0, 0, L1),
                           fig0(9, 1, 0, 0, b"\x01"))]
    c["nine short entries"] = [fib(fig0(1, 0, 0, 0, b"".join(fig01_short(k, 11 * k, k & 1, 7 * k) for k in range(9))))]
    c["long entry cut after 3"] = [fib(fig0(1, 0, 0, 0, L1 + fig01_long(6, 200, 1, 1, 21)[:3]), fig0(1, 0, 0, 0, fig01_short(7, 1, 1, 1)))]
    c["short entry cut after 2"] = [fib(fig0(1, 0, 0, 0, fig01_short(8, 300, 0, 5) + fig01_short(9, 301, 0, 6)[:2]), fig00(1, 1, 1, 2))]
    c["two FIG 0/1 in one FIB"] = [fib(fig0(1, 0, 0, 0, L1), fig0(1, 0, 0, 0, fig01_long(6, 148, 1, 3, 15)))]
    c["same SubChId twice in a FIB"] = [fib(fig0(1, 0, 0, 0, L1 + L2), fig0(1, 0, 0, 0, L1 + L2 + L2))]
    c["same SubChId in two FIBs"] = [fib(fig0(1, 0, 0, 0, L1)), fib(fig0(1, 0, 0, 0, L2))]
    c["SubChId 0 and 63"] = [fib(fig0(1, 0, 0, 0, fig01_long(0, 0, 0, 0, 12) + fig01_long(63, 1023, 7, 3, 1023) + fig01_short(63, 1023, 1, 63)),
                                 fig0(2, 0, 0, 0, fig02_service(0xFFFF, [comp(0, 0, 0, 0, 0), comp(1, 63, 63, 1, 1)], top=15)))]
    c["P/D 1"] = [fib(fig0(2, 0, 0, 1, fig02_service(0xE1C00001, [comp(0, 63, 5)], pd=1) + fig02_service(0x80000000, [], pd=1)))]
    c["TMId 0 ... 3"] = [fib(fig0(2, 0, 0, 0, fig02_service(0x4001, [comp(0, 63, 1), comp(1, 60, 2), comp(2, 5, 3), comp(3, 9, 4)])))]
    c["nc one more than fits"] = [fib(fig0(2, 0, 0, 0, fig02_service(0x4002, [comp(0, 63, 10), comp(0, 0, 11)], nc=3)))]
    c["service header cut"] = [fib(fig0(2, 0, 0, 0, S1 + b"\x12\x35"), fig0(2, 0, 0, 1, b"\x00\x00\x00\x01"))]
    c["FIG 0/0 of 4, 5 and 3"] = [fib(fig00(0x1111, 2, 1, 0x1FFF), fig00(0x1111, 2, 1, 5, b"\x63"), fig0(0, 0, 0, 0, b"\x11\x11\xa0")),
                                  fib(fig00(0x2222, 2, 1, 6), fig00(0x1111, 2, 0, 7), fig00(0x1111, 2, 1, 8))]
    c["empty FIG 0/1 and 0/2"] = [fib(fig0(1, 0, 0, 0, b""), fig0(2, 0, 0, 0, b""))]
    c["equal and other components"] = [fib(fig0(2, 0, 0, 0, S1 + fig02_service(0x1235, [comp(0, 63, 5)]))), fib(fig0(2, 0, 0, 0, S1 + S1)),
                                       fib(fig0(2, 0, 0, 0, fig02_service(0x1234, [comp(0, 62, 5)]) + S1))]
    out = {k: (np.stack(v), None) for k, v in c.items()}
    good, contra = fib(fig0(1, 0, 0, 0, L1), fig00(0x3333, 0, 0, 9)), fib(fig0(1, 0, 0, 0, L2), fig00(0x4444, 1, 0, 10), fig0(2, 0, 0, 0, S1))
    out["flag 0 with contradicting content"] = (np.stack([good, contra, raw_fib(bytes([0 << 5 | 31]))]), np.array([1, 0, 0], np.uint8))
    return out


POOL_ORG = [fig01_long(1, 0, 0, 2, 48), fig01_long(1, 0, 0, 2, 54), fig01_long(2, 54, 0, 2, 72), fig01_long(3, 126, 1, 1, 21),
            fig01_short(4, 147, 0, 10), fig01_short(4, 147, 1, 10), fig01_long(40, 500, 0, 1, 8), fig01_long(63, 600, 0, 3, 4)]
POOL_SVC = [fig02_service(0x1001, [comp(0, 63, 1)]), fig02_service(0x1001, [comp(0, 63, 1), comp(1, 5, 3)]),
            fig02_service(0x1002, [comp(0, 63, 2)]), fig02_service(0x1009, [comp(0, 63, 2)]), fig02_service(0x1004, [comp(0, 0, 4, 0, 1)]),
            fig02_service(0x1005, [comp(2, 0, 40), comp(3, 1, 40), comp(0, 63, 40)]), fig02_service(0x1006, [])]
POOL_SVC32 = [fig02_service(0xE0001001, [comp(0, 63, 1)], pd=1), fig02_service(0xE0001063, [comp(0, 63, 63)], pd=1)]


def random_fib(rng):
    """a well-formed FIB of FIGs from the pools: sub-channels signalled again and again, now and then with another value"""
    figs, room = [], 30
    while room >= 8:
        k = int(rng.integers(0, 8))
        if k == 0:
            f = fig00(0xD220 + int(rng.integers(0, 40) == 0), int(rng.integers(0, 20) == 0), 0, int(rng.integers(0, 5000)),
                      b"\x01" * int(rng.integers(0, 2)))
        elif k in (1, 2):
            f = fig0(1, int(rng.integers(0, 12) == 0), 0, 0, b"".join(POOL_ORG[int(i)] for i in rng.integers(0, len(POOL_ORG), int(rng.integers(1, 5)))))
        elif k in (3, 4):
            f = fig0(2, 0, int(rng.integers(0, 12) == 0), 0, b"".join(POOL_SVC[int(i)] for i in rng.integers(0, len(POOL_SVC), int(rng.integers(1, 4)))))
        elif k == 5:
            f = fig0(2, 0, 0, 1, POOL_SVC32[int(rng.integers(0, 2))])
        elif k == 6:
            f = fig(int(rng.integers(1, 8)), rng.integers(0, 256, int(rng.integers(0, 9)), dtype=np.uint8).tobytes())
        else:
            f = fig0(int(rng.integers(3, 32)), 0, 0, 0, rng.integers(0, 256, int(rng.integers(0, 6)), dtype=np.uint8).tobytes())
        if len(f) <= room:
            figs.append(f)
            room -= len(f)
        else:
            break
    return fib(*figs)


def random_fibs(rng, n):
    return np.stack([random_fib(rng) for _ in range(n)])


# ---- vit_mci_fibs_host against the model ------------------------------------------------------------------------------------
PATHS = Counter()   # of every input of this file; test_every_path_was_visited reads it last


def check_host(V, fibs, ok, G):
    want = mci_model(fibs, ok, G, PATHS)
    got = V.mci_fibs_host(fibs, G, ok)
    for name, g, w in zip(("sub", "grp", "status"), got, want):
        assert same(g, w), (name, G, np.flatnonzero(g.reshape(-1) != w.reshape(-1))[:8])
    return want


def test_directed_fibs(V):
    cases = directed()
    for name, (fibs, ok) in cases.items():
        sub, grp, st = check_host(V, fibs, ok, len(fibs))
        if name == "same SubChId in two FIBs":
            assert sub[0, 5]["org"] == PRESENT | LONG | 100 | 54 << 10 | 2 << 20 and sub[0, 5]["n_org"] == 1 and sub[0, 5]["n_org_other"] == 1
        if name == "same SubChId twice in a FIB":
            assert (sub[0, 5]["org"] >> 10) & 1023 == 54 and sub[0, 5]["n_org"] == 3 and sub[0, 5]["n_org_other"] == 2
        if name == "nine short entries":
            assert int((sub[0]["org"] != 0).sum()) == 9 and st[0] == ST_USED | ST_FIG01
        if name == "length overrun by 1":
            assert st[0] == ST_USED | ST_MALFORMED | ST_FIG01 and grp[0]["nfib_malformed"] == 1 and sub[0, 5]["n_org"] == 1
        if name == "flag 0 with contradicting content":
            assert st.tolist() == [ST_USED | ST_FIG00 | ST_FIG01, 0, 0] and grp[0]["eid"] == 0x3333 and grp[0]["nfib_used"] == 1
            assert (sub[0, 5]["org"] >> 10) & 1023 == 48 and sub[0, 5]["comp"] == 0
        if name == "FIG 0/0 of 4, 5 and 3":
            assert (grp[0]["eid"], grp[0]["cif"], grp[0]["flags"], grp[0]["n_ens_other"]) == (0x1111, 8, 1 | 2 << 1 | 1 << 3, 2)
        if name == "C/N and OE":
            assert grp[0]["n_next"] == 3 and (sub[0, 5]["org"] >> 10) & 1023 == 48 and sub[0, 5]["comp"] == 0
        if name == "nc one more than fits":
            assert st[0] & ST_MALFORMED and sub[0, 10]["n_comp"] == 1 and sub[0, 11]["n_comp"] == 1
        if name == "P/D 1":
            assert sub[0, 5]["sid"] == 0xE1C00001
    # all of them in a row at several group lengths, with and without flags (NULL: the flag-0 FIBs are read too)
    fibs = np.concatenate([f for f, _ in cases.values()])
    ok = np.concatenate([np.ones(len(f), np.uint8) if o is None else o for f, o in cases.values()])
    for G in (1, 2, 3, 12, len(fibs) - 1, len(fibs), MAX_G):
        check_host(V, fibs, ok, G)
        check_host(V, fibs, None, G)


def test_random_well_formed_fibs(V):
    rng = np.random.default_rng(11)
    fibs = random_fibs(rng, 600)
    ok = (rng.random(600) < 0.9).astype(np.uint8)
    for G in (1, 12, 64, 65, 599, 600, MAX_G):
        sub, grp, st = check_host(V, fibs, ok, G)
    assert not (st & ST_MALFORMED).any() and grp[0]["nfib_used"] == int(ok.sum())
    assert sub["n_org_other"].any() and sub["n_comp_other"].any() and grp["n_ens_other"].any() and grp["n_next"].any()


def test_random_bytes(V):
    """2000 FIBs of uniformly random bytes, every one used: the walk agrees with the model on garbage"""
    rng = np.random.default_rng(12)
    fibs = rng.integers(0, 256, (2000, 32), dtype=np.uint8)
    for G in (12, 2000):
        sub, grp, st = check_host(V, fibs, np.ones(2000, np.uint8), G)
    assert (st & ST_MALFORMED).any() and (st & ST_FIG01).any() and (st == ST_USED).any()


def test_arguments(V):
    L = V.lib()
    fibs = np.zeros((2, 32), np.uint8)
    sub, grp, st = np.full(64 * 20, 0xEE, np.uint8), np.full(16, 0xEE, np.uint8), np.full(2, 0xEE, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for G in (0, MAX_G + 1):
        assert L.vit_mci_fibs_host(p(fibs), None, 2, G, p(sub), p(grp), p(st)) == 1
    assert L.vit_mci_fibs_host(None, None, 2, 2, p(sub), p(grp), p(st)) == 1
    assert L.vit_mci_fibs_host(p(fibs), None, 2, 2, None, p(grp), p(st)) == 1
    assert L.vit_mci_fibs_host(p(fibs), None, 2, 2, p(sub), None, p(st)) == 1
    assert L.vit_mci_fibs_host(p(fibs), None, -1, 2, p(sub), p(grp), p(st)) == 1
    assert "vit_mci_fibs_host: bad arguments" in V.last_error()
    assert L.vit_mci_fibs_host(None, None, 0, 2, None, None, None) == 0
    assert (sub == 0xEE).all() and (grp == 0xEE).all() and (st == 0xEE).all()
    assert L.vit_mci_fibs_host(p(fibs), None, 2, MAX_G, p(sub), p(grp), None) == 0   # status is optional
    assert not sub.any() and grp.view(MCI_GROUP_DTYPE)[0]["nfib_used"] == 2
    import torch
    want = 1 if torch.cuda.is_available() else 2  # VIT_ERR_ARG / VIT_ERR_NO_DEVICE: nothing is launched either way
    assert L.vit_mci_fibs_dev(None, None, 2, 2, None, None, None, None) == want


def test_every_path_was_visited(V):
    """runs last in this file: the union of the model's path counters over the inputs above holds every label"""
    if not PATHS:  # selected alone
        test_directed_fibs(V)
        test_random_well_formed_fibs(V)
        test_random_bytes(V)
    assert set(PATHS) <= LABELS, set(PATHS) - LABELS
    assert not LABELS - set(PATHS), sorted(LABELS - set(PATHS))
    d = Counter()
    for fibs, ok in directed().values():
        mci_model(fibs, ok, len(fibs), d)
    assert set(d) == LABELS, sorted(LABELS - set(d))  # the directed FIBs alone do it


# ---- vit_eep_profile ------------------------------------------------------------------------------------------------------
KEEP_PI = [(1 << (8 + i + 1)) - 1 for i in range(24)]   # synthetic: the lowest 8+i+1 bits
KEEP_TAIL = "1100" * 6
UNIT = {0: (12, 8, 6, 4), 1: (27, 21, 18, 15)}


def eep_rule(option, level, n):
    """(L1, L2, PI1, PI2) of the header's rule"""
    if option == 1:
        return (24 * n - 3, 3) + ((10, 9), (6, 5), (4, 3), (2, 1))[level]
    return {0: (6 * n - 3, 3, 24, 23), 1: (5, 1, 13, 12) if n == 1 else (2 * n - 3, 4 * n + 3, 14, 13), 2: (6 * n - 3, 3, 8, 7),
            3: (4 * n - 3, 2 * n + 3, 3, 2)}[level]


def test_eep_profile_every_level_and_size(V):
    tail = sum(1 << i for i, ch in enumerate(KEEP_TAIL) if ch == "1")
    count = 0
    for option in (0, 1):
        bits = (192, 768)[option]
        for level in range(4):
            for n in range(1, 9216 // bits + 1):
                size = UNIT[option][level] * n
                prof, fb = V.eep_profile(option, level, size, KEEP_PI, KEEP_TAIL)
                l1, l2, p1, p2 = eep_rule(option, level, n)
                assert fb == bits * n and prof.nsegs == 3 and 32 * (l1 + l2) == fb
                assert [(prof.seg[k].steps, prof.seg[k].keep) for k in range(3)] == [(32 * l1, KEEP_PI[p1 - 1]), (32 * l2, KEEP_PI[p2 - 1]), (6, tail)]
                assert all(prof.seg[k].steps == 0 and prof.seg[k].keep == 0 for k in range(3, 8))
                assert V.punctured_length(prof, fb) == 64 * size, (option, level, n)
                count += 1
    assert count == 4 * 48 + 4 * 12


def test_eep_profile_errors(V):
    for args in ((2, 0, 12), (0, 4, 12), (0, 0, 0), (0, 0, 13), (0, 2, 5), (1, 1, 20), (0, 0, 12 * 49), (1, 3, 15 * 13), (0, 3, 4 * 49),
                 (7, 3, 1023)):
        with pytest.raises(V.ViterbiError, match="vit_eep_profile: bad arguments"):
            V.eep_profile(*args, KEEP_PI, KEEP_TAIL)
    V.eep_profile(0, 0, 12 * 48, KEEP_PI, KEEP_TAIL)
    V.eep_profile(1, 3, 15 * 12, KEEP_PI, KEEP_TAIL)
    for i, bad in ((0, 0xFF), (0, 0x3FF), (23, 0x7FFFFFFF), (10, KEEP_PI[9])):
        pi = list(KEEP_PI)
        pi[i] = bad
        with pytest.raises(V.ViterbiError, match="one bits"):
            V.eep_profile(0, 2, 6, pi, KEEP_TAIL)
    for tail in ("1100" * 5 + "1000", "1100" * 5 + "1110", 0x01FFF000, 0x1000FFE):
        with pytest.raises(V.ViterbiError, match="one bits"):
            V.eep_profile(0, 2, 6, KEEP_PI, tail)
    L = V.lib()
    pi = np.array(KEEP_PI, np.uint32)
    out, fb = V.PunctProfile(), C.c_uint32(0)
    assert L.vit_eep_profile(0, 2, 6, pi.ctypes.data_as(C.c_void_p), 0x333333, None, C.byref(fb)) == 1
    assert L.vit_eep_profile(0, 2, 6, pi.ctypes.data_as(C.c_void_p), 0x333333, C.byref(out), None) == 1
    assert L.vit_eep_profile(0, 2, 6, None, 0x333333, C.byref(out), C.byref(fb)) == 1
    assert L.vit_eep_profile(0, 2, 6, pi.ctypes.data_as(C.c_void_p), 0x333333, C.byref(out), C.byref(fb)) == 0 and fb.value == 192


# ---- vit_mci_ens_table --------------------------------------------------------------------------------------------------
def multiplex_fibs():
    """a hand-written multiplex in three FIBs (one FIC frame of 768 bits): DAB+ at EEP 3-A in sub-channels 1 (48 CU), 2
    (72 CU) and 3 (48 CU again), packet data at EEP 2-B in 5, DAB audio in short form in 7, and 9 without a component"""
    a = fib(fig00(0xD220, 0, 0, 0x0345),
            fig0(1, 0, 0, 0, fig01_long(1, 0, 0, 2, 48) + fig01_long(2, 48, 0, 2, 72) + fig01_long(5, 120, 1, 1, 21) +
                 fig01_long(3, 300, 0, 2, 48) + fig01_short(7, 141, 0, 10)))
    b = fib(fig0(1, 0, 0, 0, fig01_long(9, 200, 0, 2, 6)),
            fig0(2, 0, 0, 0, fig02_service(0x1001, [comp(0, 63, 1)]) + fig02_service(0x1002, [comp(0, 63, 2)]) +
                 fig02_service(0x1003, [comp(0, 63, 3)])))
    c = fib(fig0(2, 0, 0, 0, fig02_service(0x2001, [comp(1, 5, 5)]) + fig02_service(0x2002, [comp(0, 0, 7)])))
    return np.stack([a, b, c])


def multiplex_rows(V):
    """what vit_mci_ens_table must make of it: (rows, profiles, skipped)"""
    p48, _ = V.eep_profile(0, 2, 48, KEEP_PI, KEEP_TAIL)
    p72, _ = V.eep_profile(0, 2, 72, KEEP_PI, KEEP_TAIL)
    p2b, _ = V.eep_profile(1, 1, 21, KEEP_PI, KEEP_TAIL)
    rows = np.zeros(4, V.ENS_SUBCH_DTYPE)
    rows["col"], rows["profile"], rows["framebits"] = [0, 64 * 48, 64 * 300, 64 * 120], [0, 1, 0, 2], [1536, 2304, 1536, 768]
    rows["RSDims"], rows["nsym"] = [8, 12, 8, 0], [64 * 48, 64 * 72, 64 * 48, 64 * 21]
    return rows, [p48, p72, p2b], 1 << 7 | 1 << 9


def test_ens_table_of_a_hand_written_multiplex(V):
    sub, grp, st = V.mci_fibs_host(multiplex_fibs(), 3)
    assert same(sub, mci_model(multiplex_fibs(), None, 3)[0]) and grp[0]["eid"] == 0xD220 and grp[0]["cif"] == 0x0345
    rows, profs, skipped = V.mci_ens_table(sub[0], KEEP_PI, KEEP_TAIL)
    want_rows, want_profs, want_skipped = multiplex_rows(V)
    assert same(rows, want_rows), (rows, want_rows)
    assert [bytes(p) for p in profs] == [bytes(p) for p in want_profs] and skipped == want_skipped
    for r in rows:
        assert V.punctured_length(profs[r["profile"]], int(r["framebits"])) == r["nsym"]
    with pytest.raises(V.ViterbiError):
        V.ensemble_layout(rows)          # nframes is still the caller's to fill
    rows["nframes"] = 5
    lay = V.ensemble_layout(rows)
    assert lay["nrec"] == 3 and lay["max_framebits"] == 2304 and lay["rows_needed"] == 20
    # capacity: three profiles are needed
    _, p3, _ = V.mci_ens_table(sub[0], KEEP_PI, KEEP_TAIL, max_profiles=3)
    assert len(p3) == 3
    with pytest.raises(V.ViterbiError, match="needs one more"):
        V.mci_ens_table(sub[0], KEEP_PI, KEEP_TAIL, max_profiles=2)
    with pytest.raises(V.ViterbiError, match="one bits"):
        V.mci_ens_table(sub[0], KEEP_PI[:23] + [0], KEEP_TAIL)
    # option > 1 and a size the rule rejects are skipped, nothing signalled gives nothing
    odd = np.zeros(64, MCI_SUBCH_DTYPE)
    odd["comp"][[4, 6]] = PRESENT | 63 << 2
    odd["org"][4] = PRESENT | LONG | 2 << 22 | 2 << 20 | 48 << 10
    odd["org"][6] = PRESENT | LONG | 2 << 20 | 47 << 10
    rows, profs, skipped = V.mci_ens_table(odd, KEEP_PI, KEEP_TAIL)
    assert len(rows) == 0 and len(profs) == 0 and skipped == 1 << 4 | 1 << 6
    rows, profs, skipped = V.mci_ens_table(np.zeros(64, MCI_SUBCH_DTYPE), KEEP_PI, KEEP_TAIL)
    assert len(rows) == 0 and len(profs) == 0 and skipped == 0
