"""CPU: the service directory (include/viterbi_amd.h, "Service directory") - a pure-Python model of the FIB walk, of the
choice of the 64 smallest keys and of last-wins per group that names every path it takes, the builders of FIG 0/3 and of
the label FIGs (tests/test_gpu_mci_dir.py imports both), vit_mci_dir_host against the model in every byte, and the two
host-only steps behind it: vit_mci_dir_ens_table and vit_mci_pkt_table.

The model goes forward through a group's entries and compares each with the last one of its key and kind; the library's
host twin goes backward, the kernel by rounds of atomics.  The constants of the format stand once, below."""
import ctypes as C
import os
import sys
from collections import Counter

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from test_mci_host import (KEEP_PI, KEEP_TAIL, MAX_G, MCI_SUBCH_DTYPE, comp, fib, fig, fig0, fig00, fig01_long, fig02_service,  # noqa: E402
                           multiplex_fibs, multiplex_rows, raw_fib, same)

# ---- the format (the library's: csrc/vit_fig_fmt.h) ---------------------------------------------------------------------
DIR_MAX = 64
SERVICE_DTYPE = np.dtype([("sid", "<u4"), ("label", "u1", (16,)), ("chars", "<u2"), ("flags", "u1"), ("count", "u1"),
                          ("n_label", "<u2"), ("n_label_other", "<u2"), ("n_listed", "<u2"), ("n_listed_other", "<u2")])
PKTCOMP_DTYPE = np.dtype([("scid", "<u2"), ("flags", "<u2"), ("loc", "<u4"), ("sid", "<u4"), ("n_loc", "<u2"),
                          ("n_loc_other", "<u2"), ("n_comp", "<u2"), ("n_comp_other", "<u2")])
DIR_DTYPE = np.dtype([("eid", "<u2"), ("chars", "<u2"), ("label", "u1", (16,)), ("flags", "u1"), ("charset", "u1"),
                      ("n_label", "<u2"), ("n_label_other", "<u2"), ("nsvc", "<u2"), ("npkt", "<u2"), ("nfib_used", "<u2"),
                      ("nfib_malformed", "<u2"), ("n_next", "<u2"), ("reserved", "<u2", (2,))])
assert (SERVICE_DTYPE.itemsize, PKTCOMP_DTYPE.itemsize, DIR_DTYPE.itemsize) == (32, 20, 40)
ST_USED, ST_MALFORMED, ST_FIG02, ST_FIG03, ST_FIG1 = 1, 2, 4, 8, 16
SVC_LABEL, SVC_LISTED = 1, 2            # vit_mci_service.flags; bit 2 P/D, bits 7..4 charset
PKT_LOC, PKT_COMP = 1, 2                # vit_mci_pktcomp.flags; bit 2 P/S, bit 3 CA
DIR_LABEL, DIR_SVC_OVERFLOW, DIR_PKT_OVERFLOW = 1, 2, 4

# every path of the model; the tests below must visit them all
LABELS = frozenset("""fib_unused fib_used end_marker_at_0 end_marker ran_to_30 overrun len0 type_2_to_7 fig0_ext_other
fig1_ext_other cn_set oe_set fig1_flag_set fig0_no_entries fig02_sid16 fig02_sid32 fig02_header_cut fig02_comp_cut fig02_nc0
tmid0 tmid1 tmid2 tmid3 fig03_plain fig03_caorg fig03_cut_below_5 fig03_caorg_cut label_ens label_sid16 label_sid32 label_short
label_exact label_long svc_first svc_equal svc_other label_first label_equal label_other comp_first comp_equal comp_other
loc_first loc_equal loc_other elabel_first elabel_equal elabel_other group_without_elabel sid_overflow scid_overflow
sid_fits scid_fits entry_without_record label32_on_sid16 comp_without_loc loc_without_comp comp_and_loc service_without_label
label_without_service service_and_label""".split())


# ---- the model --------------------------------------------------------------------------------------------------------
def walk_model(b, paths):
    """one used FIB (30 bytes at least) -> (status, n_next, entries); an entry is (kind, key, value, note): ('svc', SId,
    (P/D, count byte)), ('label', SId, (label, chars, charset)), ('comp', SCId, (SId, P/S, CA)), ('loc', SCId, loc) or
    ('elabel', 0, (EId, label, chars, charset)); note is the extension of a label FIG"""
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
        elif typ >= 2:
            paths["type_2_to_7"] += 1
        elif typ == 1:
            t = b[p + 1]
            ext = t & 7
            if ext not in (0, 1, 5):
                paths["fig1_ext_other"] += 1
            elif t & 8:
                paths["fig1_flag_set"] += 1
                n_next += 1
            else:
                st |= ST_FIG1
                idlen = 4 if ext == 5 else 2
                if ln < 1 + idlen + 18:
                    paths["label_short"] += 1
                    st |= ST_MALFORMED
                else:
                    paths["label_exact" if ln == 1 + idlen + 18 else "label_long"] += 1
                    q = p + 2 + idlen
                    ident = int.from_bytes(bytes(b[p + 2:q]), "big")
                    lab, chars = bytes(b[q:q + 16]), b[q + 16] << 8 | b[q + 17]
                    if ext == 0:
                        paths["label_ens"] += 1
                        out.append(("elabel", 0, (ident, lab, chars, t >> 4), ext))
                    else:
                        paths["label_sid16" if ext == 1 else "label_sid32"] += 1
                        out.append(("label", ident, (lab, chars, t >> 4), ext))
        else:
            t = b[p + 1]
            ext, q, e = t & 31, p + 2, p + 1 + ln
            if ext not in (2, 3):
                paths["fig0_ext_other"] += 1
            elif t & 0xC0:
                if t & 0x80:
                    paths["cn_set"] += 1
                if t & 0x40:
                    paths["oe_set"] += 1
                n_next += 1
            elif ext == 2:
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
                    count = b[q + nsid]
                    out.append(("svc", sid, (pd, count), None))
                    q += nsid + 1
                    if count & 15 == 0:
                        paths["fig02_nc0"] += 1
                    for _ in range(count & 15):
                        if e - q < 2:
                            paths["fig02_comp_cut"] += 1
                            st |= ST_MALFORMED
                            leave = True
                            break
                        c0, c1 = b[q], b[q + 1]
                        paths["tmid%d" % (c0 >> 6)] += 1
                        if c0 >> 6 == 3:
                            out.append(("comp", (c0 & 63) << 6 | c1 >> 2, (sid, (c1 >> 1) & 1, c1 & 1), None))
                        q += 2
            else:
                st |= ST_FIG03
                if q == e:
                    paths["fig0_no_entries"] += 1
                while q < e:
                    if e - q < 5:
                        paths["fig03_cut_below_5"] += 1
                        st |= ST_MALFORMED
                        break
                    b0, b1, b2, b3, b4 = b[q:q + 5]
                    caorg = b1 & 1
                    if caorg and e - q < 7:
                        paths["fig03_caorg_cut"] += 1
                        st |= ST_MALFORMED
                        break
                    paths["fig03_caorg" if caorg else "fig03_plain"] += 1
                    loc = (b3 >> 2) | ((b3 & 3) << 8 | b4) << 6 | (b2 & 63) << 16 | (b2 >> 7) << 22 | caorg << 23
                    out.append(("loc", b0 << 4 | b1 >> 4, loc, None))
                    q += 7 if caorg else 5
        p += 1 + ln
    return st, n_next, out


def dir_model(fibs, ok, G, paths=None, memo=None):
    """-> (SERVICE_DTYPE (ngroups, 64), PKTCOMP_DTYPE (ngroups, 64), DIR_DTYPE (ngroups,), status bytes) by the definition
    of the header.  memo: a dict that keeps the walk of every distinct FIB (its paths are then counted once)"""
    paths = Counter() if paths is None else paths
    fibs = np.asarray(fibs, np.uint8).reshape(-1, 32)
    n = fibs.shape[0]
    ng = (n + G - 1) // G
    svc, pkt = np.zeros((ng, DIR_MAX), SERVICE_DTYPE), np.zeros((ng, DIR_MAX), PKTCOMP_DTYPE)
    grp, status = np.zeros(ng, DIR_DTYPE), np.zeros(n, np.uint8)
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
        D = grp[g]
        index = {}
        for table, kinds, flag, name in (("sid", ("svc", "label"), DIR_SVC_OVERFLOW, "nsvc"), ("scid", ("comp", "loc"), DIR_PKT_OVERFLOW, "npkt")):
            keys = sorted({k for kind, k, _, _ in ents if kind in kinds})
            if len(keys) > DIR_MAX:
                paths[table + "_overflow"] += 1
                D["flags"] |= flag
            elif keys:
                paths[table + "_fits"] += 1
            D[name] = min(len(keys), DIR_MAX)
            for i, k in enumerate(keys[:DIR_MAX]):
                index[(table, k)] = i
                (svc if table == "sid" else pkt)[g, i]["sid" if table == "sid" else "scid"] = k
        table_of = {"svc": "sid", "label": "sid", "comp": "scid", "loc": "scid", "elabel": "ens"}
        index[("ens", 0)] = 0
        last = {}
        for kind, k, v, _ in ents:
            last[(kind, k)] = v
        met = set()
        for kind, k, v, note in ents:
            i = index.get((table_of[kind], k))
            if i is None:
                paths["entry_without_record"] += 1
                continue
            w = last[(kind, k)]
            paths[kind + ("_first" if (kind, k) not in met else "_equal" if v == w else "_other")] += 1
            met.add((kind, k))
            which = "" if v == w else "_other"
            if kind == "svc":
                r = svc[g, i]
                r["flags"] = (r["flags"] & 0xF1) | SVC_LISTED | w[0] << 2
                r["count"] = w[1]
                r["n_listed" + which] += 1
            elif kind == "label":
                r = svc[g, i]
                r["flags"] = (r["flags"] & 0x0E) | SVC_LABEL | w[2] << 4
                r["label"], r["chars"] = np.frombuffer(w[0], np.uint8), w[1]
                r["n_label" + which] += 1
                if note == 5 and k < 65536 and last.get(("svc", k), (1,))[0] == 0:
                    paths["label32_on_sid16"] += 1
            elif kind == "comp":
                r = pkt[g, i]
                r["flags"] = (r["flags"] & PKT_LOC) | PKT_COMP | w[1] << 2 | w[2] << 3
                r["sid"] = w[0]
                r["n_comp" + which] += 1
            elif kind == "loc":
                r = pkt[g, i]
                r["flags"] |= PKT_LOC
                r["loc"] = w
                r["n_loc" + which] += 1
            else:
                D["eid"], D["label"], D["chars"], D["charset"] = w[0], np.frombuffer(w[1], np.uint8), w[2], w[3]
                D["flags"] |= DIR_LABEL
                D["n_label" + which] += 1
        if ("elabel", 0) not in last:
            paths["group_without_elabel"] += 1
        for r in pkt[g, :D["npkt"]]:
            paths[{PKT_LOC: "loc_without_comp", PKT_COMP: "comp_without_loc", PKT_LOC | PKT_COMP: "comp_and_loc"}[r["flags"] & 3]] += 1
        for r in svc[g, :D["nsvc"]]:
            paths[{SVC_LABEL: "label_without_service", SVC_LISTED: "service_without_label", 3: "service_and_label"}[r["flags"] & 3]] += 1
        D["nfib_used"], D["nfib_malformed"], D["n_next"] = used, malf, nxt
    return svc, pkt, grp, status


# ---- builders ---------------------------------------------------------------------------------------------------------
def loc_entry(scid, sub, addr, dscty=5, dg=1, caorg=0, rfa=0, ca=b"\xca\xfe"):
    return bytes([scid >> 4, (scid & 15) << 4 | rfa << 1 | caorg, dg << 7 | dscty, sub << 2 | addr >> 8, addr & 255]) + (bytes(ca) if caorg else b"")


def fig03(*entries, cn=0, oe=0):
    return fig0(3, cn, oe, 0, b"".join(entries))


def label16(text):
    return text.encode("ascii").ljust(16)[:16]


def fig1(ext, ident, text, chars=0xFF00, charset=0, flag=0, extra=b""):
    return fig(1, bytes([charset << 4 | flag << 3 | ext]) + ident.to_bytes(4 if ext == 5 else 2, "big") + label16(text) +
               bytes([chars >> 8, chars & 255]) + bytes(extra))


def pcomp(scid, ps=1, ca=0):
    """a TMId-3 component of FIG 0/2"""
    return bytes([3 << 6 | scid >> 6, (scid & 63) << 2 | ps << 1 | ca])


def many_sids(n, start=0x4000, step=3):
    """FIBs with n distinct 16-bit SIds in descending order, nine services a FIB"""
    sids = [start + step * k for k in range(n)][::-1]
    return [fib(fig0(2, 0, 0, 0, b"".join(fig02_service(s, [], top=s & 7) for s in sids[i:i + 9]))) for i in range(0, n, 9)]


def many_scids(n, start=7, step=61):
    """FIBs with n distinct SCIds in descending order: alternately five locations, and a service with twelve components"""
    scids, out, i = [(start + step * k) & 4095 for k in range(n)][::-1], [], 0
    assert len(set(scids)) == n
    while i < n:
        if len(out) & 1:
            out.append(fib(fig03(*[loc_entry(s, s & 63, s & 1023) for s in scids[i:i + 5]])))
            i += 5
        else:
            out.append(fib(fig0(2, 0, 0, 0, fig02_service(0x5000 + i, [pcomp(s) for s in scids[i:i + 12]]))))
            i += 12
    return out


def directed():
    """name -> (FIBs (k, 32), their flags or None): one case per path of the walk, of the choice of keys and of last-wins"""
    S1 = fig02_service(0x1234, [pcomp(0x155)])
    L1, L2 = loc_entry(0x155, 9, 5), loc_entry(0x155, 9, 700, dscty=60, dg=0)
    c = {}
    c["FIG 0/2 alone"] = [fib(fig0(2, 0, 0, 0, S1))]
    c["FIG 0/3 alone"] = [fib(fig03(L1))]
    c["FIG 1/0 alone"] = [fib(fig1(0, 0xD220, "An Ensemble"))]
    c["FIG 1/1 alone"] = [fib(fig1(1, 0x1234, "Radio One", 0xE000, 1))]
    c["FIG 1/5 alone"] = [fib(fig1(5, 0xE1C00001, "Data Service", 0x8001, 15))]
    c["C/N, OE and the label flag"] = [fib(fig0(2, 1, 0, 0, S1), fig0(2, 0, 1, 0, S1), fig03(L1, cn=1), fig03(L2, oe=1)),
                                       fib(fig1(0, 1, "next", flag=1)), fib(fig1(1, 2, "next", flag=1)), fib(fig1(5, 3, "next", flag=1)),
                                       fib(fig0(2, 0, 0, 0, S1), fig03(L1))]
    c["FIG 0/3 with and without CAOrg"] = [fib(fig03(L1, loc_entry(0x156, 10, 1023, caorg=1, rfa=7), loc_entry(0x157, 63, 0, 63)))]
    c["FIG 0/3 cut at 4 bytes"] = [fib(fig03(L1, L2[:4]), fig03(loc_entry(0x158, 1, 1)))]
    c["FIG 0/3 CAOrg cut at 6 bytes"] = [fib(fig03(L1, loc_entry(0x159, 2, 2, caorg=1)[:6]), fig03(loc_entry(0x15A, 3, 3)))]
    c["label one byte short"] = [raw_fib(bytes([1 << 5 | 20]) + fig1(1, 0x1234, "Short")[1:21] + fig0(2, 0, 0, 0, S1))]
    c["label one byte long"] = [fib(fig1(1, 0x1234, "Long", extra=b"\x77"), fig0(2, 0, 0, 0, S1))]
    c["16-bit SId as a FIG 1/5 identifier"] = [fib(fig0(2, 0, 0, 0, fig02_service(0x1234, []))), fib(fig1(5, 0x1234, "One key space", charset=6))]
    c["SId 0 and 0xFFFFFFFF"] = [fib(fig0(2, 0, 0, 0, fig02_service(0, [pcomp(0)])), fig0(2, 0, 0, 1, fig02_service(0xFFFFFFFF, [pcomp(4095, 0, 1)], pd=1, top=15))),
                                 fib(fig1(1, 0, "Zero")), fib(fig1(5, 0xFFFFFFFF, "All ones", 0xFFFF, 15)),
                                 fib(fig03(loc_entry(0, 0, 0, 0, 0), loc_entry(4095, 63, 1023, 63, 1)))]
    for n in (63, 64, 65):
        c["%d SIds" % n] = many_sids(n) + [fib(fig1(1, 0x4000 + 3 * (n - 1), "the largest")), fib(fig1(1, 0x4000, "the smallest"))]
        c["%d SCIds" % n] = many_scids(n)
    c["component without location and the reverse"] = [fib(fig0(2, 0, 0, 0, fig02_service(0x2001, [pcomp(0x200), pcomp(0x201)])),
                                                           fig03(loc_entry(0x201, 4, 40), loc_entry(0x202, 4, 41)))]
    c["13 entries"] = [fib(fig0(2, 0, 0, 0, fig02_service(0x2002, [pcomp(0x300 + k, k & 1, k >> 3) for k in range(12)])))]
    c["9 services"] = [fib(fig0(2, 0, 0, 0, b"".join(fig02_service(0x2100 + k, []) for k in range(9))))]
    c["5 locations"] = [fib(fig03(*[loc_entry(0x400 + k, k, k) for k in range(5)]))]
    c["end marker at byte 0"] = [raw_fib(b"\xff" + fig0(2, 0, 0, 0, S1))]
    full = [fig0(2, 0, 0, 0, S1), fig03(L1), fig0(2, 0, 0, 1, fig02_service(0xE0000001, [pcomp(1), pcomp(2), pcomp(3)], pd=1)), fig(2, bytes(2))]
    assert len(b"".join(full)) == 30
    c["30 bytes, no marker"] = [fib(*full)]
    c["length overrun by 1"] = [raw_fib(fig03(L1) + bytes([1 << 5 | 23, 1]) + bytes(21))]
    c["len == 0 headers"] = [raw_fib(bytes([0x00, 0x20, 0xE0]) + fig03(L1) + b"\x00\xff")]
    c["types 2 ... 7"] = [fib(*[fig(t, bytes([0x02, 0x14])) for t in range(2, 8)], fig03(L1))]
    c["other extensions"] = [fib(fig0(0, 0, 0, 0, bytes(4)), fig0(1, 0, 0, 0, fig01_long(5, 100, 0, 2, 48)), fig0(13, 0, 0, 1, S1),
                                 fig(1, bytes([4]) + bytes(5)), fig(1, bytes([7]))), fib(fig(1, bytes([2]) + bytes(20)))]
    c["service header cut"] = [fib(fig0(2, 0, 0, 0, S1 + b"\x12\x35"), fig0(2, 0, 0, 1, b"\x00\x00\x00\x01"))]
    c["nc one more than fits"] = [fib(fig0(2, 0, 0, 0, fig02_service(0x2003, [pcomp(0x500), pcomp(0x501)], nc=3)))]
    c["TMId 0 ... 3"] = [fib(fig0(2, 0, 0, 0, fig02_service(0x2004, [comp(0, 63, 1), comp(1, 60, 2), comp(2, 5, 3), pcomp(0x502)])))]
    c["empty FIG 0/2 and 0/3"] = [fib(fig0(2, 0, 0, 0, b""), fig03())]
    c["equal and other entries"] = [fib(fig0(2, 0, 0, 0, S1 + fig02_service(0x1234, [pcomp(0x155)], top=1)), fig03(L1, L2)),
                                    fib(fig1(1, 0x1234, "Radio One")), fib(fig1(1, 0x1234, "Radio 1")), fib(fig1(1, 0x1234, "Radio One", 0xFF00, 1)),
                                    fib(fig1(1, 0x1234, "Radio One", 0xFE00)), fib(fig1(1, 0x1234, "Radio One")),
                                    fib(fig0(2, 0, 0, 0, fig02_service(0x1235, [pcomp(0x155)]) + S1), fig03(L1, L1)),
                                    fib(fig0(2, 0, 0, 1, fig02_service(0x1234, [pcomp(0x155, 0)], pd=1)), fig0(2, 0, 0, 0, S1 + S1))]
    c["ensemble labels"] = [fib(fig1(0, 0xD220, "An Ensemble")), fib(fig1(0, 0xD221, "An Ensemble")), fib(fig1(0, 0xD220, "An ensemble")),
                            fib(fig1(0, 0xD220, "An Ensemble", charset=2)), fib(fig1(0, 0xD220, "An Ensemble"))]
    out = {k: (np.stack(v), None) for k, v in c.items()}
    good, contra = fib(fig03(L1), fig0(2, 0, 0, 0, S1)), fib(fig03(L2), fig0(2, 0, 0, 0, fig02_service(0x9999, [pcomp(0x155)])))
    out["flag 0 with contradicting content"] = (np.stack([good, contra, raw_fib(bytes([0 << 5 | 31]))]), np.array([1, 0, 0], np.uint8))
    return out


NAMES = ["Radio %d" % k for k in range(20)]
POOL_SVC = ([fig02_service(0x1000 + k, [comp(0, 63, k)]) for k in range(1, 18)] +
            [fig02_service(0x1012, [pcomp(0x101)]), fig02_service(0x1013, [pcomp(0x102, 0)]), fig02_service(0x1013, [pcomp(0x102, 0), pcomp(0x103)]),
             fig02_service(0x1012, [pcomp(0x101, 1, 1)], top=2)])
POOL_LOC = [loc_entry(0x101, 9, 5), loc_entry(0x102, 9, 700), loc_entry(0x102, 9, 701), loc_entry(0x103, 10, 1, caorg=1)]


def random_fib(rng):
    """a well-formed FIB of a multiplex of twenty services: services, labels and packet components signalled again and
    again, now and then with another value"""
    figs, room = [], 30
    while room >= 7:
        k = int(rng.integers(0, 8))
        if k == 0 and room >= 22:
            s = int(rng.integers(0, 20))
            f = fig1(1, 0x1000 + s, NAMES[s] if rng.integers(0, 30) else "Radio?", flag=int(rng.integers(0, 25) == 0))
        elif k == 1 and room >= 24:
            f = (fig1(5, 0xE0001001, "Data") if rng.integers(0, 2) else fig1(0, 0xD220 + int(rng.integers(0, 40) == 0), "The Ensemble",
                                                                             extra=b"\x01" * int(rng.integers(0, 2))))
        elif k in (2, 3, 4):
            f = fig0(2, 0, int(rng.integers(0, 12) == 0), 0, b"".join(POOL_SVC[int(i)] for i in rng.integers(0, len(POOL_SVC), int(rng.integers(1, 4)))))
        elif k == 5:
            f = fig03(*[POOL_LOC[int(i)] for i in rng.integers(0, len(POOL_LOC), int(rng.integers(1, 3)))], cn=int(rng.integers(0, 12) == 0))
        elif k == 6:
            f = fig0(2, 0, 0, 1, fig02_service(0xE0001001, [pcomp(0x103)], pd=1))
        else:
            typ = int(rng.integers(0, 8))   # passed over: FIG 0/4 ... 0/31, FIG 1/2 and 1/6, types 2 ... 7
            f = fig(typ, bytes([int(rng.integers(4, 32)) if typ != 1 else (0x12, 0x06)[int(rng.integers(0, 2))]]) +
                    rng.integers(0, 256, int(rng.integers(0, 5)), dtype=np.uint8).tobytes())
        if len(f) <= room:
            figs.append(f)
            room -= len(f)
        else:
            break
    return fib(*figs)


def random_fibs(rng, n):
    return np.stack([random_fib(rng) for _ in range(n)])


# ---- vit_mci_dir_host against the model -------------------------------------------------------------------------------------
PATHS = Counter()   # of every input of this file; test_every_path_was_visited reads it last
NAMES_OUT = ("svc", "pkt", "dir", "status")


def check_host(V, fibs, ok, G):
    want = dir_model(fibs, ok, G, PATHS)
    got = V.mci_dir_host(fibs, G, ok)
    for name, g, w in zip(NAMES_OUT, got, want):
        assert same(g, w), (name, G, np.flatnonzero(g.view(np.uint8).reshape(-1) != w.view(np.uint8).reshape(-1))[:8])
    return want


def test_record_layouts(V):
    assert V.MCI_SERVICE_DTYPE == SERVICE_DTYPE and V.MCI_PKTCOMP_DTYPE == PKTCOMP_DTYPE and V.MCI_DIR_DTYPE == DIR_DTYPE


def test_directed_fibs(V):
    cases = directed()
    for name, (fibs, ok) in cases.items():
        svc, pkt, d, st = check_host(V, fibs, ok, len(fibs))
        d = d[0]
        if name == "FIG 1/1 alone":
            assert bytes(svc[0, 0]["label"]) == b"Radio One       " and svc[0, 0]["flags"] == SVC_LABEL | 1 << 4 and svc[0, 0]["chars"] == 0xE000
            assert d["nsvc"] == 1 and d["npkt"] == 0 and st[0] == ST_USED | ST_FIG1
        if name == "FIG 0/3 alone":
            assert pkt[0, 0]["scid"] == 0x155 and pkt[0, 0]["loc"] == 9 | 5 << 6 | 5 << 16 | 1 << 22 and pkt[0, 0]["flags"] == PKT_LOC
        if name == "C/N, OE and the label flag":
            assert d["n_next"] == 7 and d["nsvc"] == 1 and d["npkt"] == 1 and not d["flags"]
        if name == "FIG 0/3 cut at 4 bytes":
            assert st[0] == ST_USED | ST_MALFORMED | ST_FIG03 and d["npkt"] == 2
        if name == "FIG 0/3 CAOrg cut at 6 bytes":
            assert st[0] & ST_MALFORMED and pkt[0, :2]["scid"].tolist() == [0x155, 0x15A] and d["npkt"] == 2
        if name == "label one byte short":
            assert st[0] == ST_USED | ST_MALFORMED | ST_FIG1 | ST_FIG02 and svc[0, 0]["flags"] == SVC_LISTED
        if name == "label one byte long":
            assert st[0] == ST_USED | ST_FIG1 | ST_FIG02 and svc[0, 0]["flags"] == SVC_LISTED | SVC_LABEL
        if name == "16-bit SId as a FIG 1/5 identifier":
            assert d["nsvc"] == 1 and svc[0, 0]["flags"] == SVC_LISTED | SVC_LABEL | 6 << 4 and svc[0, 0]["sid"] == 0x1234
        if name == "SId 0 and 0xFFFFFFFF":
            assert svc[0, :2]["sid"].tolist() == [0, 0xFFFFFFFF] and (svc[0, :2]["flags"] & 7).tolist() == [3, 7] and d["nsvc"] == 2
            assert pkt[0, :2]["scid"].tolist() == [0, 4095] and (pkt[0, :2]["flags"]).tolist() == [3 | 4, 3 | 8] and d["npkt"] == 2
            assert pkt[0, 1]["sid"] == 0xFFFFFFFF and pkt[0, 1]["loc"] == 0x7FFFFF and svc[0, 1]["count"] == 0xF1
        for n in (63, 64, 65):
            if name == "%d SIds" % n:
                assert d["nsvc"] == min(n, 64) and d["flags"] == (DIR_SVC_OVERFLOW if n > 64 else 0)
                assert svc[0, :64]["sid"].tolist() == [0x4000 + 3 * k for k in range(min(n, 64))] + [0] * (64 - min(n, 64))
                assert svc[0, 0]["flags"] & SVC_LABEL and bool(svc[0, min(n, 64) - 1]["flags"] & SVC_LABEL) == (n <= 64)
            if name == "%d SCIds" % n:
                assert d["npkt"] == min(n, 64) and d["flags"] == (DIR_PKT_OVERFLOW if n > 64 else 0)
                assert pkt[0, :d["npkt"]]["scid"].tolist() == sorted((7 + 61 * k) & 4095 for k in range(n))[:64]
        if name == "component without location and the reverse":
            assert (pkt[0, :3]["flags"] & 3).tolist() == [PKT_COMP, PKT_COMP | PKT_LOC, PKT_LOC] and pkt[0, 2]["sid"] == 0 and pkt[0, 0]["loc"] == 0
        if name == "13 entries":
            assert d["nsvc"] == 1 and d["npkt"] == 12 and svc[0, 0]["count"] == 12
        if name == "equal and other entries":
            r, p = svc[0, 0], pkt[0, 0]
            assert (r["n_listed"], r["n_listed_other"], r["n_label"], r["n_label_other"]) == (4, 2, 2, 3)
            assert (p["n_comp"], p["n_comp_other"], p["n_loc"], p["n_loc_other"]) == (5, 2, 3, 1) and p["loc"] & 63 == 9
        if name == "ensemble labels":
            assert (d["eid"], d["n_label"], d["n_label_other"], d["charset"], d["flags"]) == (0xD220, 2, 3, 0, DIR_LABEL)
        if name == "flag 0 with contradicting content":
            assert st.tolist() == [ST_USED | ST_FIG02 | ST_FIG03, 0, 0] and d["nfib_used"] == 1 and pkt[0, 0]["sid"] == 0x1234
    # all of them in a row at several group lengths, with and without flags (NULL: the flag-0 FIBs are read too)
    fibs = np.concatenate([f for f, _ in cases.values()])
    ok = np.concatenate([np.ones(len(f), np.uint8) if o is None else o for f, o in cases.values()])
    for G in (1, 2, 3, 12, len(fibs) - 1, len(fibs), MAX_G):
        check_host(V, fibs, ok, G)
        check_host(V, fibs, None, G)


def test_random_well_formed_fibs(V):
    rng = np.random.default_rng(31)
    fibs = random_fibs(rng, 600)
    ok = (rng.random(600) < 0.9).astype(np.uint8)
    for G in (1, 12, 64, 65, 599, 600, MAX_G):
        svc, pkt, d, st = check_host(V, fibs, ok, G)
    assert not (st & ST_MALFORMED).any() and d[0]["nfib_used"] == int(ok.sum()) and d[0]["nsvc"] == 21 and d[0]["npkt"] == 3
    assert svc["n_label_other"].any() and svc["n_listed_other"].any() and pkt["n_loc_other"].any() and pkt["n_comp_other"].any()
    assert d["n_label_other"].any() and d["n_next"].any()


def random_bytes(rng, n):
    """n FIBs of uniformly random bytes; three in four of them start with the header of one of the FIGs that are read (a
    FIG of uniformly random bytes is one of them once in a hundred), so that a group holds many distinct keys"""
    fibs = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    heads = np.array([[0, 0x02], [0, 0x22], [0, 0x03], [1, 0x01], [1, 0x05], [1, 0x00]])[rng.integers(0, 6, n)]
    forced = rng.random(n) < 0.75
    fibs[forced, 0] = (heads[forced, 0] << 5) | (fibs[forced, 0] & 31)
    fibs[forced, 1] = heads[forced, 1] | (fibs[forced, 1] & 0x10)
    return fibs


def test_random_bytes(V):
    """2000 FIBs of random bytes, every one used: the walk agrees with the model on garbage, and the many distinct keys of
    a long group meet the overflow rule"""
    fibs = random_bytes(np.random.default_rng(32), 2000)
    for G in (12, 2000):
        svc, pkt, d, st = check_host(V, fibs, np.ones(2000, np.uint8), G)
    assert (st & ST_MALFORMED).any() and (st & ST_FIG03).any() and (st == ST_USED).any()
    assert d[0]["flags"] & DIR_SVC_OVERFLOW and d[0]["flags"] & DIR_PKT_OVERFLOW and d[0]["nsvc"] == 64 and d[0]["npkt"] == 64


def test_two_runs_give_the_same_bytes(V):
    fibs = random_fibs(np.random.default_rng(33), 300)
    a, b = V.mci_dir_host(fibs, 100), V.mci_dir_host(fibs, 100)
    assert all(same(x, y) for x, y in zip(a, b))


def test_arguments(V):
    L = V.lib()
    fibs = np.zeros((2, 32), np.uint8)
    svc, pkt, d, st = (np.full(n, 0xEE, np.uint8) for n in (64 * 32, 64 * 20, 40, 2))
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for G in (0, MAX_G + 1):
        assert L.vit_mci_dir_host(p(fibs), None, 2, G, p(svc), p(pkt), p(d), p(st)) == 1
    assert L.vit_mci_dir_host(None, None, 2, 2, p(svc), p(pkt), p(d), p(st)) == 1
    assert L.vit_mci_dir_host(p(fibs), None, 2, 2, None, p(pkt), p(d), p(st)) == 1
    assert L.vit_mci_dir_host(p(fibs), None, 2, 2, p(svc), None, p(d), p(st)) == 1
    assert L.vit_mci_dir_host(p(fibs), None, 2, 2, p(svc), p(pkt), None, p(st)) == 1
    assert L.vit_mci_dir_host(p(fibs), None, -1, 2, p(svc), p(pkt), p(d), p(st)) == 1
    assert "vit_mci_dir_host: bad arguments" in V.last_error()
    assert L.vit_mci_dir_host(None, None, 0, 2, None, None, None, None) == 0
    assert all((a == 0xEE).all() for a in (svc, pkt, d, st))
    assert L.vit_mci_dir_host(p(fibs), None, 2, MAX_G, p(svc), p(pkt), p(d), None) == 0   # status is optional
    assert not svc.any() and not pkt.any() and d.view(DIR_DTYPE)[0]["nfib_used"] == 2
    import torch
    want = 1 if torch.cuda.is_available() else 2  # VIT_ERR_ARG / VIT_ERR_NO_DEVICE: nothing is launched either way
    assert L.vit_mci_dir_dev(None, None, 2, 2, None, None, None, None, None) == want


def test_every_path_was_visited(V):
    """runs last among the model's tests: the union of the model's path counters over the inputs above holds every label"""
    if not PATHS:  # selected alone
        test_directed_fibs(V)
        test_random_well_formed_fibs(V)
        test_random_bytes(V)
    assert set(PATHS) <= LABELS, set(PATHS) - LABELS
    assert not LABELS - set(PATHS), sorted(LABELS - set(PATHS))
    d = Counter()
    for fibs, ok in directed().values():
        dir_model(fibs, ok, len(fibs), d)
    assert set(d) == LABELS, sorted(LABELS - set(d))  # the directed FIBs alone do it


# ---- vit_mci_dir_ens_table, vit_mci_pkt_table ------------------------------------------------------------------------------
def packet_multiplex_fibs():
    """multiplex_fibs() of tests/test_mci_host.py - DAB+ in sub-channels 1, 2 and 3, a data component with TMId 1 in 5, DAB
    audio in short form in 7 - whose sub-channel 9 (EEP 3-A, 6 CU: 24 bytes a frame, no component in FIG 0/2's eyes) now
    carries packet mode: two service components at addresses 5 and 700, and the names"""
    d = fib(fig0(2, 0, 0, 0, fig02_service(0x3001, [pcomp(0x101)]) + fig02_service(0x3002, [pcomp(0x102, 0)])),
            fig03(loc_entry(0x101, 9, 5, dscty=60), loc_entry(0x102, 9, 700, dscty=5)))
    e = [fib(fig1(0, 0xD220, "Hand Written Mux")), fib(fig1(1, 0x1001, "Radio One")), fib(fig1(1, 0x3001, "Slides")),
         fib(fig1(1, 0x3002, "Traffic", 0xFE00))]
    return np.concatenate([multiplex_fibs(), np.stack([d] + e)])


def packet_multiplex_rows(V):
    """what vit_mci_dir_ens_table must make of it: (rows, profiles, skipped, packet_rows)"""
    rows, profs, skipped = multiplex_rows(V)
    p6, _ = V.eep_profile(0, 2, 6, KEEP_PI, KEEP_TAIL)
    more = np.zeros(1, V.ENS_SUBCH_DTYPE)
    more["col"], more["profile"], more["framebits"], more["nsym"] = 64 * 200, 3, 192, 64 * 6
    return np.concatenate([rows, more]), profs + [p6], skipped & ~(1 << 9), 1 << 4


def test_tables_of_a_hand_written_multiplex(V):
    fibs = packet_multiplex_fibs()
    sub, _, _ = V.mci_fibs_host(fibs, len(fibs))
    svc, pkt, d, _ = V.mci_dir_host(fibs, len(fibs))
    assert same(svc, dir_model(fibs, None, len(fibs))[0]) and d[0]["npkt"] == 2 and d[0]["nsvc"] == 7
    assert bytes(d[0]["label"]) == b"Hand Written Mux" and d[0]["eid"] == 0xD220
    npkt = int(d[0]["npkt"])
    rows, profs, skipped, marked = V.mci_dir_ens_table(sub[0], pkt[0, :npkt], KEEP_PI, KEEP_TAIL)
    want = packet_multiplex_rows(V)
    assert same(rows, want[0]), (rows, want[0])
    assert [bytes(p) for p in profs] == [bytes(p) for p in want[1]] and skipped == want[2] and marked == want[3]
    # an address finds its service and its name: packet record -> SId -> service record
    by_addr = {(int(r["loc"]) >> 6) & 1023: r for r in pkt[0, :npkt] if r["flags"] & PKT_LOC and r["loc"] & 63 == 9}
    names = {int(r["sid"]): bytes(r["label"]).rstrip() for r in svc[0, :d[0]["nsvc"]] if r["flags"] & SVC_LABEL}
    assert names[int(by_addr[5]["sid"])] == b"Slides" and names[int(by_addr[700]["sid"])] == b"Traffic"
    # npkt == 0: vit_mci_ens_table's outputs, on this multiplex and on the one without packet mode
    for f in (fibs, multiplex_fibs()):
        s0 = V.mci_fibs_host(f, len(f))[0][0]
        r0, p0, k0 = V.mci_ens_table(s0, KEEP_PI, KEEP_TAIL)
        r1, p1, k1, m1 = V.mci_dir_ens_table(s0, None, KEEP_PI, KEEP_TAIL)
        assert same(r0, r1) and [bytes(p) for p in p0] == [bytes(p) for p in p1] and k0 == k1 and m1 == 0
    r0, _, k0 = V.mci_ens_table(sub[0], KEEP_PI, KEEP_TAIL)
    assert same(r0, multiplex_rows(V)[0]) and k0 == 1 << 7 | 1 << 9
    # a record without bit 0, and one that names a sub-channel with a component, add nothing
    odd = pkt[0, :npkt].copy()
    odd["flags"] &= ~np.uint16(PKT_LOC)
    odd2 = pkt[0, :1].copy()
    odd2["loc"] = (odd2["loc"] & ~np.uint32(63)) | 5
    for o in (odd, odd2):
        r1, _, k1, m1 = V.mci_dir_ens_table(sub[0], o, KEEP_PI, KEEP_TAIL)
        assert same(r1, r0) and k1 == k0 and m1 == 0
    # the rows pass vit_ensemble_layout, the stream table vit_packet_table_layout
    rows["nframes"] = 5
    lay = V.ensemble_layout(rows)
    for fec, score in ((V.PKT_FEC_NONE, 0), (V.PKT_FEC_SEARCH, 0), (V.PKT_FEC_SEARCH, 7)):
        tab, row_of = V.mci_pkt_table(rows, lay, marked, fec, score)
        assert row_of.tolist() == [4] and len(tab) == 1
        assert (tab[0]["offset"], tab[0]["framebytes"], tab[0]["nframes"], tab[0]["fec"], tab[0]["phase"], tab[0]["min_score"], tab[0]["reserved"]) == \
            (lay["work_offset"][4], 24, 5, fec, 0, score, 0)
        pl = V.packet_table_layout(tab)
        assert pl["nrec"] == 5 and pl["bytes_end"] == lay["work_offset"][4] + 120 <= lay["work_bytes"]
    # two packet sub-channels: streams in row order
    two = sub[0].copy()
    two[5]["comp"] = 0
    pk = pkt[0, :npkt].copy()
    pk[0]["loc"] = (pk[0]["loc"] & ~np.uint32(63)) | 5
    rows2, _, k2, m2 = V.mci_dir_ens_table(two, pk, KEEP_PI, KEEP_TAIL)
    assert m2 == 1 << 3 | 1 << 4 and k2 == 1 << 7
    rows2["nframes"] = 10
    lay2 = V.ensemble_layout(rows2)
    tab, row_of = V.mci_pkt_table(rows2, lay2, m2, V.PKT_FEC_SEARCH, 3)
    assert row_of.tolist() == [3, 4] and tab["framebytes"].tolist() == [96, 24] and tab["offset"].tolist() == [lay2["work_offset"][3], lay2["work_offset"][4]]
    V.packet_table_layout(tab)
    assert len(V.mci_pkt_table(rows2, lay2, 0)[0]) == 0


def test_table_argument_errors(V):
    L = V.lib()
    fibs = packet_multiplex_fibs()
    sub = V.mci_fibs_host(fibs, len(fibs))[0][0]
    svc, pkt, d, _ = V.mci_dir_host(fibs, len(fibs))
    rows, profs, skipped, marked = V.mci_dir_ens_table(sub, pkt[0, :2], KEEP_PI, KEEP_TAIL)
    with pytest.raises(V.ViterbiError, match="needs one more"):
        V.mci_dir_ens_table(sub, pkt[0, :2], KEEP_PI, KEEP_TAIL, max_profiles=3)
    with pytest.raises(V.ViterbiError, match="one bits"):
        V.mci_dir_ens_table(sub, pkt[0, :2], KEEP_PI[:23] + [0], KEEP_TAIL)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    pi = np.array(KEEP_PI, np.uint32)
    out, prof = np.zeros(64, V.ENS_SUBCH_DTYPE), (V.PunctProfile * 64)()
    n, npf, sk, mk = C.c_uint32(0), C.c_uint32(64), C.c_uint64(0), C.c_uint64(0)
    good = [p(sub), p(pkt), 2, p(pi), 0x333333, p(out), C.byref(n), C.byref(prof), C.byref(npf), C.byref(sk), C.byref(mk)]
    assert L.vit_mci_dir_ens_table(*good) == 0 and n.value == 5 and mk.value == 1 << 4
    for k in (0, 1, 3, 5, 6, 7, 8, 9, 10):
        bad = list(good)
        bad[k] = None
        assert L.vit_mci_dir_ens_table(*bad) == 1, k
    bad = list(good)
    bad[2] = 65
    assert L.vit_mci_dir_ens_table(*bad) == 1 and "vit_mci_dir_ens_table: bad arguments" in V.last_error()
    bad[1], bad[2] = None, 0
    npf.value = 64
    assert L.vit_mci_dir_ens_table(*bad) == 0 and mk.value == 0 and n.value == 4
    # vit_mci_pkt_table
    rows["nframes"] = 5
    lay = V.ensemble_layout(rows)
    V.mci_pkt_table(rows, lay, marked)
    for kw in (dict(fec=V.PKT_FEC_PHASE), dict(fec=3), dict(fec=V.PKT_FEC_NONE, min_score=1)):
        with pytest.raises(V.ViterbiError, match="vit_mci_pkt_table: bad arguments"):
            V.mci_pkt_table(rows, lay, marked, **kw)
    with pytest.raises(V.ViterbiError, match="at or above nsub"):
        V.mci_pkt_table(rows, lay, 1 << 5)
    with pytest.raises(V.ViterbiError, match="row 0"):
        V.mci_pkt_table(rows, lay, 1)            # a DAB+ row is no packet stream
    for field, value in (("framebits", 200), ("framebits", 192 * 49), ("framebits", 8), ("nframes", 0)):
        r = rows.copy()
        r[4][field] = value
        with pytest.raises(V.ViterbiError, match="row 4"):
            V.mci_pkt_table(r, lay, marked)
    tab, ns, lay1 = np.zeros(64, V.PKT_STREAM_DTYPE), C.c_uint32(0), np.asarray(lay).reshape(1)
    good = [p(rows), 5, p(lay1), marked, 0, 0, p(tab), C.byref(ns), None]
    assert L.vit_mci_pkt_table(*good) == 0 and ns.value == 1      # the row numbers are optional
    for k in (0, 2, 6, 7):
        bad = list(good)
        bad[k] = None
        assert L.vit_mci_pkt_table(*bad) == 1, k
    for nsub in (0, 65):
        bad = list(good)
        bad[1] = nsub
        assert L.vit_mci_pkt_table(*bad) == 1
