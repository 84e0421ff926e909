"""GPU: the multiplex configuration (vit_mci_fibs_dev) against the model and the builders of tests/test_mci_host.py, byte
for byte: sentinel bytes around every output, the input unchanged, base offsets 0, 1 and 3 for d_fibs; the group lengths at
which the kernel changes its shape (a wavefront per group up to 64 FIBs, tiles of 256 above); and the chain from
vit_decode_fic_dev to the rows of vit_ensemble_dev."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (torch's runtime first, as when the whole suite is collected)

from test_dab_host import scramble
from test_gpu_dab import channel, dev, fic_frames, fic_profile
from test_mci_host import (KEEP_PI, KEEP_TAIL, MAX_G, MCI_GROUP_DTYPE, MCI_SUBCH_DTYPE, ST_FIG00, ST_FIG01, ST_FIG02, ST_USED,
                           directed, fib, fig0, fig01_long, mci_model, multiplex_fibs, multiplex_rows, random_fibs, same)
from test_punct_host import puncture

pytestmark = pytest.mark.gpu

SREC, GREC = MCI_SUBCH_DTYPE.itemsize, MCI_GROUP_DTYPE.itemsize  # 20, 16
TILE = 256        # FIBs of a tile of vit_mci_kernel (G > 64)
PASS_GROUPS = 4   # groups of one pass for G <= 64
MAX_GRID = 1024   # workgroups of a launch: more passes than this make a second grid-stride trip
PAD = 32
MEMO = {}         # the model's walk of every distinct FIB, shared by all cases


# ---- running ----------------------------------------------------------------------------------------------------------
def run_mci(V, torch, fibs, ok, G, offset=0, status=True):
    fibs = np.ascontiguousarray(fibs, np.uint8).reshape(-1, 32)
    n = fibs.shape[0]
    ng = (n + G - 1) // G
    host = np.concatenate([np.full(PAD, 0xC3, np.uint8), fibs.reshape(-1), np.full(PAD, 0xC3, np.uint8)])
    d = dev(host, offset)
    d_ok = None if ok is None else dev(np.concatenate([np.asarray(ok, np.uint8), np.zeros(1, np.uint8)]), 1)
    d_sub = torch.full(((64 * ng + 2) * SREC,), 0xEE, dtype=torch.uint8, device="cuda")
    d_grp = torch.full(((ng + 2) * GREC,), 0xEE, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n + 2 * PAD,), 0xEE, dtype=torch.uint8, device="cuda")
    V.mci_fibs_dev(d[PAD:], n, G, d_sub[SREC:], d_grp[GREC:], d_ok, d_st[PAD:] if status else None)
    torch.cuda.synchronize()
    sub, grp, st = d_sub.cpu().numpy(), d_grp.cpu().numpy(), d_st.cpu().numpy()
    assert (sub[:SREC] == 0xEE).all() and (sub[(64 * ng + 1) * SREC:] == 0xEE).all()
    assert (grp[:GREC] == 0xEE).all() and (grp[(ng + 1) * GREC:] == 0xEE).all()
    assert (st[:PAD] == 0xEE).all() and (st[PAD + n:] == 0xEE).all() and (status or (st == 0xEE).all())
    assert np.array_equal(d.cpu().numpy(), host)
    if ok is not None:
        assert np.array_equal(d_ok.cpu().numpy()[:n], np.asarray(ok, np.uint8))
    return (sub[SREC:(64 * ng + 1) * SREC].view(MCI_SUBCH_DTYPE).reshape(ng, 64), grp[GREC:(ng + 1) * GREC].view(MCI_GROUP_DTYPE),
            st[PAD:PAD + n] if status else None)


def check(V, torch, fibs, ok, G, offset=0, status=True):
    want = mci_model(fibs, ok, G, memo=MEMO)
    got = run_mci(V, torch, fibs, ok, G, offset, status)
    for name, g, w in zip(("sub", "grp", "status"), got, want):
        if g is not None:
            assert same(g, w), (name, G, len(fibs), offset, np.flatnonzero(g.reshape(-1) != w.reshape(-1))[:8])
    return want


@pytest.fixture(scope="module")
def pool():
    """random well-formed FIBs, a tenth of them with a failed CRC flag, and the directed FIBs among them: a stream of n FIBs
    is its first n -> (FIBs, flags)"""
    rng = np.random.default_rng(21)
    base = random_fibs(rng, 300)
    fibs = base[rng.integers(0, 300, 4200)]
    ok = (rng.random(4200) < 0.9).astype(np.uint8)
    at = 0
    for dfibs, dok in directed().values():
        for rep in range(2):  # near the front (every shape sees them) and spread out
            pos = at if rep == 0 else 150 + 37 * at
            fibs[pos:pos + len(dfibs)] = dfibs
            ok[pos:pos + len(dfibs)] = 1 if dok is None else dok
        at += len(dfibs)
    assert at < 60
    return fibs, ok


# ---- the shapes ---------------------------------------------------------------------------------------------------------
SHAPES = [
    # G, nfibs: one group, two, and five with a partial last one
    (12, 12), (12, 24), (12, 50), (3, 14), (1, 1), (1, 5),
    # the lengths around one wavefront per group, and around one tile
    (63, 5 * 63 - 7), (64, 5 * 64 - 7), (65, 5 * 65 - 7), (TILE - 1, 2 * TILE + 98), (TILE, 2 * TILE + 100), (TILE + 1, 2 * TILE + 102),
    (600, 1500), (MAX_G, MAX_G + 1), (MAX_G, 700),
    # below, at and above what one trip of the grid takes: the first workgroup makes a second pass
    (1, PASS_GROUPS * MAX_GRID - 1), (1, PASS_GROUPS * MAX_GRID), (1, PASS_GROUPS * MAX_GRID + 1),
]


@pytest.mark.parametrize("G,nfibs", SHAPES)
def test_against_the_model(V, torch_cuda, pool, G, nfibs):
    fibs, ok = pool[0][:nfibs], pool[1][:nfibs]
    offset = (0, 1, 3)[(G + nfibs) % 3]
    sub, grp, st = check(V, torch_cuda, fibs, ok, G, offset)
    if nfibs >= 60:
        assert sub["n_org_other"].any() and sub["n_comp"].any() and (grp["flags"] & 1).any() and (st == 0).any()


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
    for pos in (0, 64 - k, 64, 127, TILE - k, TILE, 2 * TILE - k):
        fibs[pos:pos + k] = dfibs
        ok[pos:pos + k] = 1 if dok is None else dok
    for G in (2 * TILE, 64):
        _, _, st = check(V, torch_cuda, fibs, ok, G, 1)
        assert (st[TILE - k:TILE] == mci_model(dfibs, dok, k)[2]).all()


def test_conflict_across_a_tile_boundary_twice(V, torch_cuda):
    """SubChId 5 with one value in the last FIB of a tile and another in the first FIB of the next: the later FIB wins, and
    two runs give the same bytes"""
    rng = np.random.default_rng(5)
    fibs = random_fibs(rng, 40)[rng.integers(0, 40, 3 * TILE)]
    fibs[TILE - 1] = fib(fig0(1, 0, 0, 0, fig01_long(5, 100, 0, 2, 48)))
    fibs[TILE] = fib(fig0(1, 0, 0, 0, fig01_long(5, 100, 0, 2, 54)))
    fibs[TILE + 1:] = fib(fig0(1, 0, 0, 0, fig01_long(6, 200, 0, 2, 6)))
    fibs[:TILE - 1] = fibs[TILE + 1]
    runs = [run_mci(V, torch_cuda, fibs, None, 3 * TILE, 3) for _ in range(2)]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs))
    want = mci_model(fibs, None, 3 * TILE, memo=MEMO)
    assert all(same(g, w) for g, w in zip(runs[0], want))
    r = runs[0][0][0, 5]
    assert (r["org"] >> 10) & 1023 == 54 and r["n_org"] == 1 and r["n_org_other"] == 1 and runs[0][0][0, 6]["n_org"] == 3 * TILE - 2


# ---- arguments ------------------------------------------------------------------------------------------------------------
def test_argument_errors(V, torch_cuda):
    torch = torch_cuda
    L = V.lib()
    d = torch.full((64,), 0x11, dtype=torch.uint8, device="cuda")
    o = torch.full((64 * SREC + GREC + 8,), 0xEE, dtype=torch.uint8, device="cuda")
    st = torch.full((8,), 0xEE, dtype=torch.uint8, device="cuda")
    fibs, sub, grp, stp = (C.c_void_p(t) for t in (d.data_ptr(), o.data_ptr(), o.data_ptr() + 64 * SREC, st.data_ptr()))
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.vit_mci_fibs_dev(None, None, 2, 2, sub, grp, stp, s) == 1
    assert L.vit_mci_fibs_dev(fibs, None, 2, 2, None, grp, stp, s) == 1
    assert L.vit_mci_fibs_dev(fibs, None, 2, 2, sub, None, stp, s) == 1
    for G in (0, MAX_G + 1, 0xFFFFFFFF):
        assert L.vit_mci_fibs_dev(fibs, None, 2, G, sub, grp, stp, s) == 1
    assert L.vit_mci_fibs_dev(fibs, None, -1, 2, sub, grp, stp, s) == 1
    for k in (1, 2, 3):
        assert L.vit_mci_fibs_dev(fibs, None, 2, 2, C.c_void_p(o.data_ptr() + k), grp, stp, s) == 1
        assert L.vit_mci_fibs_dev(fibs, None, 2, 2, sub, C.c_void_p(o.data_ptr() + 64 * SREC + k), stp, s) == 1
    assert "vit_mci_fibs_dev: bad arguments" in V.last_error()
    assert L.vit_mci_fibs_dev(None, None, 0, 2, None, None, None, s) == 0 and L.vit_mci_fibs_dev(fibs, None, 0, 2, sub, grp, stp, s) == 0
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


def test_fic_chain_to_the_ensemble_table(V, O, torch_cuda):
    """8 FIC frames whose FIBs carry the hand-written multiplex, one of them damaged: vit_decode_fic_dev, vit_mci_fibs_dev on
    its outputs on the same stream, one copy of 1296 bytes, vit_mci_ens_table"""
    torch = torch_cuda
    rng = np.random.default_rng(8)
    n, framebits = 8, 768
    pay = np.tile(multiplex_fibs()[None, :, :30], (n, 1, 1))
    _, frames = fic_frames(_Payloads(pay), n, framebits)
    assert np.array_equal(frames.reshape(-1, 32), np.tile(multiplex_fibs(), (n, 1)))
    sym = channel(O, scramble(frames, framebits), framebits, rng, "clean")
    sym[2, :800] = rng.integers(0, 256, 800, dtype=np.uint8)  # 200 bits: the first FIB of frame 2 does not survive
    d_in = dev(puncture(sym, fic_profile(framebits), framebits), 1)
    d_f = torch.zeros(n * 96, dtype=torch.uint8, device="cuda")
    d_ok = torch.zeros(n * 3, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(64 * SREC + GREC, dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(n * 3, dtype=torch.uint8, device="cuda")
    V.decode_fic_dev(d_in, d_f, d_ok, framebits, n, fic_profile(framebits))
    V.mci_fibs_dev(d_f, 3 * n, 3 * n, d_out, d_out[64 * SREC:], d_ok, d_st)
    out = d_out.cpu().numpy()  # (the copy synchronises)
    sub, grp = out[:64 * SREC].view(MCI_SUBCH_DTYPE), out[64 * SREC:].view(MCI_GROUP_DTYPE)[0]
    ok, st = d_ok.cpu().numpy(), d_st.cpu().numpy()
    assert ok.sum() == 3 * n - 1 and ok[6] == 0
    assert st.reshape(n, 3)[0].tolist() == [ST_USED | ST_FIG00 | ST_FIG01, ST_USED | ST_FIG01 | ST_FIG02, ST_USED | ST_FIG02] and st[6] == 0
    want = mci_model(d_f.cpu().numpy().reshape(-1, 32), ok, 3 * n)
    assert same(sub.reshape(1, 64), want[0]) and grp.tobytes() == want[1].tobytes()
    assert (grp["eid"], grp["cif"], grp["nfib_used"], grp["nfib_malformed"]) == (0xD220, 0x0345, 3 * n - 1, 0)
    assert sub[1]["n_org"] == n - 1 and sub[9]["n_org"] == n and sub[5]["n_comp"] == n and not sub["n_org_other"].any()
    rows, profs, skipped = V.mci_ens_table(sub, KEEP_PI, KEEP_TAIL)
    want_rows, want_profs, want_skipped = multiplex_rows(V)
    assert same(rows, want_rows) and [bytes(p) for p in profs] == [bytes(p) for p in want_profs] and skipped == want_skipped
