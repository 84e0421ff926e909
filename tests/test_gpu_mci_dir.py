"""GPU: the service directory (vit_mci_dir_dev) against the model and the builders of tests/test_mci_dir_host.py, byte for
byte: sentinel bytes around every output, the input unchanged, base offsets for d_fibs; the group lengths at which the
kernel changes its shape (a wavefront per group up to 64 FIBs, tiles of 256 above, a second sweep above one tile); keys
that arrive tile by tile; and the chain from vit_decode_fic_dev to the rows and the packet streams."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (torch's runtime first, as when the whole suite is collected)

from test_dab_host import scramble
from test_gpu_dab import channel, dev, fic_frames, fic_profile
from test_gpu_mci import SHAPES, TILE
from test_mci_dir_host import (DIR_DTYPE, DIR_PKT_OVERFLOW, DIR_SVC_OVERFLOW, PKTCOMP_DTYPE, SERVICE_DTYPE, ST_FIG1, ST_FIG02, ST_FIG03,
                               ST_USED, dir_model, directed, fig1, fig03, loc_entry, many_scids, many_sids, packet_multiplex_fibs,
                               packet_multiplex_rows, pcomp, random_fibs)
from test_mci_host import KEEP_PI, KEEP_TAIL, MAX_G, MCI_GROUP_DTYPE, MCI_SUBCH_DTYPE, fib, fig0, fig02_service, same
from test_punct_host import puncture

pytestmark = pytest.mark.gpu

VREC, PREC, DREC = SERVICE_DTYPE.itemsize, PKTCOMP_DTYPE.itemsize, DIR_DTYPE.itemsize  # 32, 20, 40
PAD = 32
MEMO = {}         # the model's walk of every distinct FIB, shared by all cases
NAMES = ("svc", "pkt", "dir", "status")


# ---- running ----------------------------------------------------------------------------------------------------------
def run_dir(V, torch, fibs, ok, G, offset=0, status=True):
    fibs = np.ascontiguousarray(fibs, np.uint8).reshape(-1, 32)
    n = fibs.shape[0]
    ng = (n + G - 1) // G
    host = np.concatenate([np.full(PAD, 0xC3, np.uint8), fibs.reshape(-1), np.full(PAD, 0xC3, np.uint8)])
    d = dev(host, offset)
    d_ok = None if ok is None else dev(np.concatenate([np.asarray(ok, np.uint8), np.zeros(1, np.uint8)]), 1)
    d_svc = torch.full(((64 * ng + 2) * VREC,), 0xEE, dtype=torch.uint8, device="cuda")
    d_pkt = torch.full(((64 * ng + 2) * PREC,), 0xEE, dtype=torch.uint8, device="cuda")
    d_dir = torch.full(((ng + 2) * DREC,), 0xEE, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n + 2 * PAD,), 0xEE, dtype=torch.uint8, device="cuda")
    V.mci_dir_dev(d[PAD:], n, G, d_svc[VREC:], d_pkt[PREC:], d_dir[DREC:], d_ok, d_st[PAD:] if status else None)
    torch.cuda.synchronize()
    svc, pkt, dr, st = d_svc.cpu().numpy(), d_pkt.cpu().numpy(), d_dir.cpu().numpy(), d_st.cpu().numpy()
    for a, rec, k in ((svc, VREC, 64 * ng), (pkt, PREC, 64 * ng), (dr, DREC, ng)):
        assert (a[:rec] == 0xEE).all() and (a[(k + 1) * rec:] == 0xEE).all()
    assert (st[:PAD] == 0xEE).all() and (st[PAD + n:] == 0xEE).all() and (status or (st == 0xEE).all())
    assert np.array_equal(d.cpu().numpy(), host)
    if ok is not None:
        assert np.array_equal(d_ok.cpu().numpy()[:n], np.asarray(ok, np.uint8))
    return (svc[VREC:(64 * ng + 1) * VREC].view(SERVICE_DTYPE).reshape(ng, 64), pkt[PREC:(64 * ng + 1) * PREC].view(PKTCOMP_DTYPE).reshape(ng, 64),
            dr[DREC:(ng + 1) * DREC].view(DIR_DTYPE), st[PAD:PAD + n] if status else None)


def check(V, torch, fibs, ok, G, offset=0, status=True):
    want = dir_model(fibs, ok, G, memo=MEMO)
    got = run_dir(V, torch, fibs, ok, G, offset, status)
    for name, g, w in zip(NAMES, got, want):
        if g is not None:
            assert same(g, w), (name, G, len(fibs), offset, np.flatnonzero(g.view(np.uint8).reshape(-1) != w.view(np.uint8).reshape(-1))[:8])
    return want


@pytest.fixture(scope="module")
def pool():
    """random well-formed FIBs, a tenth of them with a failed CRC flag, and the directed FIBs among them: a stream of n FIBs
    is its first n -> (FIBs, flags)"""
    rng = np.random.default_rng(41)
    base = random_fibs(rng, 300)
    fibs = base[rng.integers(0, 300, 4200)]
    ok = (rng.random(4200) < 0.9).astype(np.uint8)
    at = 0
    for dfibs, dok in directed().values():
        for rep in range(2):  # near the front (every shape sees some) and spread out
            pos = at if rep == 0 else 300 + 19 * at
            fibs[pos:pos + len(dfibs)] = dfibs
            ok[pos:pos + len(dfibs)] = 1 if dok is None else dok
        at += len(dfibs)
    assert at < 200
    return fibs, ok


# ---- the shapes (those of tests/test_gpu_mci.py: the kernel keeps that kernel's shape) ------------------------------------
@pytest.mark.parametrize("G,nfibs", SHAPES)
def test_against_the_model(V, torch_cuda, pool, G, nfibs):
    fibs, ok = pool[0][:nfibs], pool[1][:nfibs]
    offset = (0, 1, 3)[(G + nfibs) % 3]
    svc, pkt, d, st = check(V, torch_cuda, fibs, ok, G, offset)
    if nfibs >= 300:
        assert svc["n_label"].any() and svc["n_listed_other"].any() and pkt["n_loc"].any() and pkt["n_comp"].any() and (st == 0).any()
    if G >= 600:
        assert d[0]["flags"] & DIR_SVC_OVERFLOW and d[0]["flags"] & DIR_PKT_OVERFLOW and d[0]["flags"] & 1


@pytest.mark.parametrize("G,nfibs,offset", [(12, 50, 0), (64, 200, 1), (TILE + 1, 2 * TILE + 102, 3), (MAX_G, MAX_G + 1, 1)])
def test_optional_arguments(V, torch_cuda, pool, G, nfibs, offset):
    """d_fib_ok NULL (every FIB is used) and d_status NULL, each alone and together"""
    fibs, ok = pool[0][:nfibs], pool[1][:nfibs]
    check(V, torch_cuda, fibs, None, G, offset)
    check(V, torch_cuda, fibs, ok, G, offset, status=False)
    check(V, torch_cuda, fibs, None, G, offset, status=False)


def test_every_base_offset(V, torch_cuda, pool):
    for G, nfibs in ((12, 50), (600, 700)):
        for offset in (0, 1, 3, 16, 29):
            check(V, torch_cuda, pool[0][:nfibs], pool[1][:nfibs], G, offset)


@pytest.mark.parametrize("name", sorted(directed()))
def test_directed_fibs_at_the_edges(V, torch_cuda, name):
    """the case at the first and the last lane of a wavefront and at the first and the last FIB of a tile (a case of k
    FIBs ends or starts there, and once lies across two wavefronts), in a group of two tiles and in groups of one wavefront"""
    dfibs, dok = directed()[name]
    rng = np.random.default_rng(len(name))
    fibs = random_fibs(rng, 40)[rng.integers(0, 40, 2 * TILE)]
    ok = np.ones(2 * TILE, np.uint8)
    k = len(dfibs)
    for pos in (0, 64 - k, 64, 128 - k // 2, TILE - k, TILE, 2 * TILE - k):
        fibs[pos:pos + k] = dfibs
        ok[pos:pos + k] = 1 if dok is None else dok
    for G in (2 * TILE, 64):
        _, _, _, st = check(V, torch_cuda, fibs, ok, G, 1)
        assert (st[TILE - k:TILE] == dir_model(dfibs, dok, k)[3]).all()


def test_conflicts_across_a_tile_boundary_twice(V, torch_cuda):
    """a service's label and a component's location with one value in the last FIB of a tile and another in the first FIB
    of the next: the later FIB wins, and two runs give the same bytes"""
    rng = np.random.default_rng(5)
    fibs = random_fibs(rng, 40)[rng.integers(0, 40, 3 * TILE)]
    fibs[TILE - 2] = fib(fig1(1, 0x7001, "Before"))
    fibs[TILE - 1] = fib(fig03(loc_entry(0x777, 9, 5)))
    fibs[TILE] = fib(fig1(1, 0x7001, "After"))
    fibs[TILE + 1] = fib(fig03(loc_entry(0x777, 9, 6)))
    fibs[TILE + 2:] = fib(fig1(1, 0x7002, "Filler"), fig03(loc_entry(0x778, 1, 1)))
    fibs[:TILE - 2] = fibs[TILE + 2]
    runs = [run_dir(V, torch_cuda, fibs, None, 3 * TILE, 3) for _ in range(2)]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs))
    want = dir_model(fibs, None, 3 * TILE, memo=MEMO)
    assert all(same(g, w) for g, w in zip(runs[0], want))
    svc, pkt = runs[0][0][0], runs[0][1][0]
    assert svc[:2]["sid"].tolist() == [0x7001, 0x7002] and bytes(svc[0]["label"]).rstrip() == b"After"
    assert (svc[0]["n_label"], svc[0]["n_label_other"], svc[1]["n_label"]) == (1, 1, 3 * TILE - 4)
    assert pkt[:2]["scid"].tolist() == [0x777, 0x778] and (pkt[0]["loc"] >> 6) & 1023 == 6 and (pkt[0]["n_loc"], pkt[0]["n_loc_other"]) == (1, 1)


@pytest.mark.parametrize("where", ["first tile", "last tile"])
@pytest.mark.parametrize("which", ["smallest", "largest"])
def test_the_65th_key_in_one_tile_only(V, torch_cuda, where, which):
    """a group of three tiles whose every tile holds the same 64 SIds and 64 SCIds; one more of each, below or above them
    all, stands in the first or the last tile only: it takes the first record or leaves only the flag"""
    base = np.stack(many_sids(64) + many_scids(64))
    fibs = base[np.arange(3 * TILE) % len(base)]
    sid, scid = (0x3000, 1) if which == "smallest" else (0xF0000000, 4094)
    assert scid not in {(7 + 61 * k) & 4095 for k in range(64)}
    pos = 100 if where == "first tile" else 2 * TILE + 100
    fibs[pos] = fib(fig0(2, 0, 0, 1, fig02_service(sid, [pcomp(scid)], pd=1)), fig03(loc_entry(scid, 3, 33)))
    svc, pkt, d, _ = check(V, torch_cuda, fibs, None, 3 * TILE, 1)
    assert d[0]["flags"] == DIR_SVC_OVERFLOW | DIR_PKT_OVERFLOW and d[0]["nsvc"] == 64 and d[0]["npkt"] == 64
    assert (svc[0, 0]["sid"] == sid) == (which == "smallest") and (pkt[0, 0]["scid"] == scid) == (which == "smallest")
    assert sid not in svc[0, 1:]["sid"] and scid not in pkt[0, 1:]["scid"]


def test_every_tile_brings_new_keys(V, torch_cuda):
    """a group of four tiles: tile t holds the SIds and SCIds 4k + t alone, 20 of each, so every tile's keys interleave
    with the others' and the 64 smallest of the 80 come from all four"""
    tiles = []
    for t in range(4):
        sids = [0x100 + 4 * k + t for k in range(20)]
        own = [fib(fig0(2, 0, 0, 0, b"".join(fig02_service(s, [pcomp(s)]) for s in sids[i:i + 4])), fig03(loc_entry(sids[i], t, i)))
               for i in range(0, 20, 4)] + [fib(fig1(1, s, "Service %d" % s)) for s in sids]
        tiles.append(np.stack(own)[np.arange(TILE) % len(own)])
    fibs = np.concatenate(tiles)
    svc, pkt, d, _ = check(V, torch_cuda, fibs, None, 4 * TILE, 3)
    assert svc[0]["sid"].tolist() == list(range(0x100, 0x140)) and pkt[0]["scid"].tolist() == list(range(0x100, 0x140))
    assert d[0]["flags"] == DIR_SVC_OVERFLOW | DIR_PKT_OVERFLOW and (svc[0]["flags"] & 3 == 3).all()
    check(V, torch_cuda, fibs, None, 4 * TILE - 1, 0)   # the same keys with the groups' boundary one FIB off the tiles'


# ---- arguments ------------------------------------------------------------------------------------------------------------
def test_argument_errors(V, torch_cuda):
    torch = torch_cuda
    L = V.lib()
    d = torch.full((64,), 0x11, dtype=torch.uint8, device="cuda")
    o = torch.full((64 * VREC + 64 * PREC + DREC + 8,), 0xEE, dtype=torch.uint8, device="cuda")
    st = torch.full((8,), 0xEE, dtype=torch.uint8, device="cuda")
    at = (o.data_ptr(), o.data_ptr() + 64 * VREC, o.data_ptr() + 64 * (VREC + PREC))
    fibs, svc, pkt, dr, stp = (C.c_void_p(t) for t in (d.data_ptr(),) + at + (st.data_ptr(),))
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.vit_mci_dir_dev(None, None, 2, 2, svc, pkt, dr, stp, s) == 1
    assert L.vit_mci_dir_dev(fibs, None, 2, 2, None, pkt, dr, stp, s) == 1
    assert L.vit_mci_dir_dev(fibs, None, 2, 2, svc, None, dr, stp, s) == 1
    assert L.vit_mci_dir_dev(fibs, None, 2, 2, svc, pkt, None, stp, s) == 1
    for G in (0, MAX_G + 1, 0xFFFFFFFF):
        assert L.vit_mci_dir_dev(fibs, None, 2, G, svc, pkt, dr, stp, s) == 1
    assert L.vit_mci_dir_dev(fibs, None, -1, 2, svc, pkt, dr, stp, s) == 1
    for k in (1, 2, 3):
        assert L.vit_mci_dir_dev(fibs, None, 2, 2, C.c_void_p(at[0] + k), pkt, dr, stp, s) == 1
        assert L.vit_mci_dir_dev(fibs, None, 2, 2, svc, C.c_void_p(at[1] + k), dr, stp, s) == 1
        assert L.vit_mci_dir_dev(fibs, None, 2, 2, svc, pkt, C.c_void_p(at[2] + k), stp, s) == 1
    assert "vit_mci_dir_dev: bad arguments" in V.last_error()
    assert L.vit_mci_dir_dev(None, None, 0, 2, None, None, None, None, s) == 0 and L.vit_mci_dir_dev(fibs, None, 0, 2, svc, pkt, dr, stp, s) == 0
    torch.cuda.synchronize()
    assert (o.cpu().numpy() == 0xEE).all() and (st.cpu().numpy() == 0xEE).all() and (d.cpu().numpy() == 0x11).all()


# ---- the chain ------------------------------------------------------------------------------------------------------------
class _Payloads:
    """stands in for the generator of fic_frames: the payloads are given"""

    def __init__(self, pay):
        self.pay = pay

    def integers(self, lo, hi, shape, dtype):
        assert tuple(shape) == self.pay.shape
        return self.pay.astype(dtype)


def test_fic_chain_to_the_packet_tables(V, O, torch_cuda):
    """8 FIC frames whose 24 FIBs carry the hand-written multiplex with its packet sub-channel (8 FIBs, three times over),
    one frame damaged: vit_decode_fic_dev, vit_mci_fibs_dev and vit_mci_dir_dev on its outputs on the same stream, one copy
    to the host, vit_mci_dir_ens_table and vit_mci_pkt_table"""
    torch = torch_cuda
    rng = np.random.default_rng(9)
    n, framebits = 8, 768
    mux = packet_multiplex_fibs()
    assert len(mux) == 8
    pay = np.tile(mux[:, :30], (3, 1)).reshape(n, 3, 30)
    _, frames = fic_frames(_Payloads(pay), n, framebits)
    assert np.array_equal(frames.reshape(-1, 32), np.tile(mux, (3, 1)))
    sym = channel(O, scramble(frames, framebits), framebits, rng, "clean")
    sym[2, :800] = rng.integers(0, 256, 800, dtype=np.uint8)  # 200 bits: the first FIB of frame 2 does not survive
    d_in = dev(puncture(sym, fic_profile(framebits), framebits), 1)
    d_f = torch.zeros(n * 96, dtype=torch.uint8, device="cuda")
    d_ok = torch.zeros(n * 3, dtype=torch.uint8, device="cuda")
    sizes = (64 * MCI_SUBCH_DTYPE.itemsize, MCI_GROUP_DTYPE.itemsize, 64 * VREC, 64 * PREC, DREC, 3 * n)
    at = np.concatenate([[0], np.cumsum(sizes)])
    d_out = torch.zeros(int(at[-1]), dtype=torch.uint8, device="cuda")
    part = [d_out[int(a):int(b)] for a, b in zip(at[:-1], at[1:])]
    V.decode_fic_dev(d_in, d_f, d_ok, framebits, n, fic_profile(framebits))
    V.mci_fibs_dev(d_f, 3 * n, 3 * n, part[0], part[1], d_ok)
    V.mci_dir_dev(d_f, 3 * n, 3 * n, part[2], part[3], part[4], d_ok, part[5])
    out = d_out.cpu().numpy()  # (the one copy; it synchronises)
    h = [out[int(a):int(b)] for a, b in zip(at[:-1], at[1:])]
    sub, svc, pkt, d, st = h[0].view(MCI_SUBCH_DTYPE), h[2].view(SERVICE_DTYPE), h[3].view(PKTCOMP_DTYPE), h[4].view(DIR_DTYPE)[0], h[5]
    ok = d_ok.cpu().numpy()
    assert ok.sum() == 3 * n - 1 and ok[6] == 0 and st[6] == 0
    assert st[8:16].tolist() ==[ST_USED, ST_USED | ST_FIG02, ST_USED | ST_FIG02, ST_USED | ST_FIG02 | ST_FIG03] + [ST_USED | ST_FIG1] * 4
    want = dir_model(d_f.cpu().numpy().reshape(-1, 32), ok, 3 * n)
    assert same(svc.reshape(1, 64), want[0]) and same(pkt.reshape(1, 64), want[1]) and d.tobytes() == want[2].tobytes()
    assert (d["eid"], d["nsvc"], d["npkt"], d["nfib_used"], d["nfib_malformed"], d["n_label"]) == (0xD220, 7, 2, 3 * n - 1, 0, 3)
    assert svc[5]["sid"] == 0x3001 and svc[5]["n_label"] == 2 and svc[5]["n_listed"] == 3   # its label's first FIB was the damaged one
    rows, profs, skipped, marked = V.mci_dir_ens_table(sub, pkt[:d["npkt"]], KEEP_PI, KEEP_TAIL)
    want_rows, want_profs, want_skipped, want_marked = packet_multiplex_rows(V)
    assert same(rows, want_rows) and [bytes(p) for p in profs] == [bytes(p) for p in want_profs]
    assert skipped == want_skipped and marked == want_marked
    rows["nframes"] = 10
    lay = V.ensemble_layout(rows)
    tab, row_of = V.mci_pkt_table(rows, lay, marked, V.PKT_FEC_SEARCH, 2)
    assert row_of.tolist() == [4] and tab[0]["offset"] == lay["work_offset"][4] and tab[0]["framebytes"] == 24 and tab[0]["nframes"] == 10
    assert V.packet_table_layout(tab)["nrec"] == 10
