"""GPU: the ensemble table kernels where tests/test_gpu_ensemble.py cannot fail - later loop trips of the persistent RS
kernels and the edges of a table's shape.  Geometry and inputs come from tests/test_ens_trips_host.py, which proves
without a GPU that they reach what is claimed here; every test asserts those preconditions again for the device it runs on.

  1. rs_table_kernel with more than twice as many passes as resident workgroups: every workgroup makes two or three trips,
     looks its next pass up in another sub-channel of another width, prefetches it while it decodes, and resets s_minfail
     / s_sum for a new number of slots.
  2. rs_kernel (the uniform call) past its first trip on the dword copy-out, the byte path and the unaligned input.
  3. vit_rs_table_dev and vit_dabplus_aus_table_dev on 64 entries, entries that are not DAB+ first, last and in a row,
     sub-channels of exactly one pass and of one superframe more, and a table without any DAB+ entry.
  4. vit_ensemble_dev on 64 entries with more frames than two workgroups of the descriptor kernel.

Large cases tile a short period of distinct superframes on the device; the oracle decodes the distinct ones only.
Buffers start as a sentinel and are compared WHOLE, as in tests/test_gpu_ensemble.py.

Not reached, and not reachable at a reasonable size: the grid-stride trips of vit_ens_post_kernel and vit_au_table_kernel.
Their grids go to 2^20 workgroups (8 frames or records each) and their loops carry no state from one trip to the next."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from test_au_host import AU_BAD_HEADER, AU_DTYPE, AU_OK, AU_RS_FAILED, au_table_model, same
from test_dab_host import fire_ok_model, scramble
from test_ens_trips_host import (EDGE_TABLES, LONE_AT, ONLY_PLAIN, UNIFORM_CASES, assert_failures_on_every_trip,
                                 assert_trip_preconditions, dab, decode_periods, edge_rs_blocks, passes, period_blocks, plain,
                                 tiled_returns, trip_facts, trips_rows, uniform_dims)
from test_gpu_au import random_batch
from test_gpu_dab import channel, dabplus_superframes, dabplus_symbols, decodable_segments, dev
from test_gpu_ensemble import (FLAG_FILL, MSC_COL, POISON, REC, RET_FILL, RS_FILL, SLACK, WORK_FILL, Outputs, assert_same_buffers,
                               dev_ring, in_work_layout, per_subchannel, table)
from test_punct_host import depuncture, puncture
from test_ti_host import CU, interleave, place_in_ring

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import rsdirect as D  # noqa: E402

pytestmark = pytest.mark.gpu

IN_FILL = 0x3C
TPB = 256  # csrc/vit_dab.hip: frames per workgroup of vit_ens_desc_kernel


def device_cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


# ---- 1., 2. later trips --------------------------------------------------------------------------------------------------

class Tiled:
    """dims: (RSDims, superframes) per entry, all DAB+.  Input on the device: every entry's period of distinct superframes
    repeated over its block of the work layout, the gaps at IN_FILL; expected d_rs_out and d_ret on the host from the
    oracle's results for the distinct superframes, the rest at the sentinels."""

    def __init__(self, V, O, dims, offset, lone=None):
        self.dims, self.offset = dims, offset
        self.rows = [dab(r, n) for r, n in dims]
        self.sub = table(V, self.rows)
        self.lay = lay = V.ensemble_layout(self.sub)
        self.m = passes(self.rows, device_cus(), lay)
        blocks = period_blocks(D.Pool(), dims, lone=lone)
        decoded = decode_periods(O, dims, blocks)
        self.ret = tiled_returns(dims, decoded)
        self.nrec, self.rs_bytes = int(lay["nrec"]), int(lay["rs_bytes"])
        self.want_rs = np.full(offset + self.rs_bytes + SLACK, RS_FILL, np.uint8)
        buf = torch.full((offset + int(lay["work_bytes"]) + SLACK,), IN_FILL, dtype=torch.uint8, device="cuda")
        self.d_work = buf[offset:]
        for k, ((r, nsf), b, (_, out)) in enumerate(zip(dims, blocks, decoded)):
            wo, ro = int(lay["work_offset"][k]), int(lay["rs_offset"][k])
            which = torch.arange(nsf, device="cuda") % b.shape[0]
            self.d_work[wo:wo + nsf * 120 * r].view(nsf, 120 * r).copy_(torch.from_numpy(b).cuda()[which])
            self.want_rs[offset + ro:offset + ro + nsf * 110 * r] = out[np.arange(nsf) % b.shape[0]].reshape(-1)
        self.want_ret = np.concatenate((self.ret, np.full(4, RET_FILL, np.int32)))
        self._rs = torch.full((offset + self.rs_bytes + SLACK,), RS_FILL, dtype=torch.uint8, device="cuda")
        self.d_rs = self._rs[offset:]
        self.d_ret = torch.full((self.nrec + 4,), RET_FILL, dtype=torch.int32, device="cuda")

    def assert_outputs(self, what):
        torch.cuda.synchronize()
        for name, got, want in (("d_rs_out", self._rs.cpu().numpy(), self.want_rs), ("d_ret", self.d_ret.cpu().numpy(), self.want_ret)):
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, "%s: %s differs from the oracle at %d places, first %s" % (what, name, bad.size, bad[:8])

    def assert_equals_uniform(self, V):
        """vit_rs_batch_dev per sub-channel on the same input bytes, at the same alignment of input and output"""
        for k, (r, nsf) in enumerate(self.dims):
            wo, ro, ri = (int(self.lay[n][k]) for n in ("work_offset", "rs_offset", "rec_index"))
            n = nsf * 110 * r
            rs = torch.full((16 + n + SLACK,), RS_FILL, dtype=torch.uint8, device="cuda")[(self.offset + ro) % 16:]
            ret = torch.full((nsf + 4,), RET_FILL, dtype=torch.int32, device="cuda")
            V.rs_batch_dev(self.d_work[wo:], rs, ret, r, nsf)
            assert torch.equal(rs[:n], self.d_rs[ro:ro + n]) and bool((rs[n:] == RS_FILL).all()), k
            assert torch.equal(ret[:nsf], self.d_ret[ri:ri + nsf]) and bool((ret[nsf:] == RET_FILL).all()), k


@pytest.mark.parametrize("offset", [0, 1])
def test_rs_table_later_trips(V, O, torch_cuda, offset):
    """offset 0: the register prefetch handed from trip to trip across widths, 16-byte and dword copy-outs; offset 1 (input
    and output): copy_linear and the byte copy-out on later trips"""
    dims = trips_rows(device_cus())
    c = Tiled(V, O, dims, offset, lone=LONE_AT)
    facts = trip_facts(c.m)
    print("rs_table_kernel on %d CUs: %s" % (device_cus(), facts))
    assert_trip_preconditions(facts)
    assert_failures_on_every_trip(c.m, c.ret, lone_rec=int(c.lay["rec_index"][LONE_AT]))
    assert c.d_work.numel() + 2 * c.d_rs.numel() < 256 << 20
    assert (c.d_work.data_ptr() & 15) == offset == (c.d_rs.data_ptr() & 15)
    V.rs_table_dev(c.d_work, c.d_rs, c.d_ret, c.sub)
    c.assert_outputs("rs table, later trips")
    c.assert_equals_uniform(V)


@pytest.mark.parametrize("r,offset", UNIFORM_CASES)
def test_rs_uniform_later_trips(V, O, torch_cuda, r, offset):
    """RSDims 12: copy_out<uint32_t> (110 * 12 = 8 mod 16); RSDims 7: 770 bytes per superframe, the byte path; RSDims 8 one
    byte off: no register prefetch, and bytes out"""
    dims = uniform_dims(r, device_cus())
    c = Tiled(V, O, dims, offset)
    m = c.m
    assert m.grid == 4 * device_cus() < m.npass and 4 * sum(len(t) >= 2 for t in m.trips) >= m.grid
    assert m.nloc[-1] < m.spb[-1] and m.trip_of[-1] == 1  # the partial pass is a second trip
    assert {int(m.trip_of[g]) for g in range(m.npass) if (c.ret[m.rec[g]:m.rec[g] + m.nloc[g]] < 0).any()} == {0, 1}
    assert (c.d_work.data_ptr() & 15) == offset == (c.d_rs.data_ptr() & 15)
    V.rs_batch_dev(c.d_work, c.d_rs, c.d_ret, r, dims[0][1])
    c.assert_outputs("uniform RS, RSDims %d offset %d" % (r, offset))


# ---- 3. table shapes -------------------------------------------------------------------------------------------------------

def filler(rows, rng):
    """blocks of random bytes for the entries that are not DAB+ (their frames in d_work)"""
    return [None if r else rng.integers(0, 256, nframes * fb // 8, dtype=np.uint8) for fb, r, nframes in rows]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("name", sorted(EDGE_TABLES))
def test_rs_table_shapes(V, O, torch_cuda, name, offset):
    rows = EDGE_TABLES[name]
    sub = table(V, rows)
    lay = V.ensemble_layout(sub)
    rs_in = edge_rs_blocks(D.Pool(), rows)
    blocks = [b if b is not None else f for b, f in zip(rs_in, filler(rows, np.random.default_rng(5)))]
    host = in_work_layout(lay, blocks)
    d_work = dev(host, offset)
    got, want = Outputs(lay, offset), Outputs(lay, offset)
    V.rs_table_dev(d_work, got.rs, got.ret, sub)
    oracle_ret = []
    for k, (_, r, nframes) in enumerate(rows):
        if not r:
            continue
        nsf = nframes // 5
        wo, ro, ri = (int(lay[n][k]) for n in ("work_offset", "rs_offset", "rec_index"))
        V.rs_batch_dev(d_work[wo:], want.rs[ro:], want.ret[ri:], r, nsf)
        ret, out = O.rs_check_batch(rs_in[k], r, np.full((nsf, 110 * r), RS_FILL, np.uint8))
        oracle_ret += ret.tolist()
        torch.cuda.synchronize()
        assert np.array_equal(want.rs[ro:ro + out.size].cpu().numpy(), out.reshape(-1)), k
    got, want = got.host(), want.host()
    assert_same_buffers(got, want, name, ("d_rs_out", "d_ret"))
    assert got[2][:len(oracle_ret)].tolist() == oracle_ret and (got[2][len(oracle_ret):] == RET_FILL).all()
    assert (got[0] == WORK_FILL).all() and (got[3] == FLAG_FILL).all() and (got[4] == FLAG_FILL).all()
    assert np.array_equal(d_work.cpu().numpy(), host)
    assert min(oracle_ret) == -1 and max(oracle_ret) >= 3, name
    if name.startswith("rsdims_1"):  # the first and the last slot of the full pass, and the superframe behind a full pass
        assert oracle_ret[0] == oracle_ret[255] == oracle_ret[256 + 256] == -1


@pytest.fixture(scope="module")
def au_cases():
    """per edge table: its superframes (None where not DAB+) and return values with failures at both ends"""
    cases = {}
    for name, rows in EDGE_TABLES.items():
        rng = np.random.default_rng(len(name) + 4 * len(rows))
        sfs = [random_batch(rng, r, nframes // 5) if r else None for _, r, nframes in rows]
        for s in sfs:
            if s is not None and s.shape[0] >= 2:
                s[1, 3:5] = 0  # the first access unit would start at 0, inside the header: AU_BAD_HEADER at any RSDims
        nrec = sum(s.shape[0] for s in sfs if s is not None)
        ret = rng.integers(0, 4, nrec).astype(np.int32)
        ret[[0, nrec // 2, nrec - 1]] = -1
        cases[name] = (sfs, ret)
    return cases


@pytest.mark.parametrize("from_work", [False, True])
@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("name", sorted(EDGE_TABLES))
def test_au_table_shapes(V, torch_cuda, au_cases, name, from_work, gated):
    rows = EDGE_TABLES[name]
    sfs, ret = au_cases[name]
    sub = table(V, rows)
    lay = V.ensemble_layout(sub)
    if from_work:  # the superframe before RS: the first 110 rows of each 120-row block
        wide = [None if s is None else np.concatenate([s, np.full((s.shape[0], s.shape[1] // 11), 0x77, np.uint8)], axis=1) for s in sfs]
        host = in_work_layout(lay, [w if w is not None else f for w, f in zip(wide, filler(rows, np.random.default_rng(6)))])
    else:
        host = np.full(int(lay["rs_bytes"]), IN_FILL, np.uint8)
        for k, s in enumerate(sfs):
            if s is not None:
                o = int(lay["rs_offset"][k])
                host[o:o + s.size] = s.reshape(-1)
    d_sf = dev(host, 1 if from_work else 0)
    d_ret = torch.from_numpy(ret).cuda() if gated else None
    want, model = Outputs(lay), []
    for k, (_, r, nframes) in enumerate(rows):
        if not r:
            continue
        nsf = nframes // 5
        o, ri = int(lay["work_offset" if from_work else "rs_offset"][k]), int(lay["rec_index"][k])
        V.dabplus_aus_dev(d_sf[o:], r, nsf, want.au[ri * REC:], d_ret=d_ret[ri:] if gated else None, sf_stride=(120 if from_work else 110) * r)
        model.append(au_table_model(sfs[k], r, ret[ri:ri + nsf] if gated else None))
    want, model = want.host(), np.concatenate(model)
    assert same(want[4][:model.size * REC].view(AU_DTYPE), model)
    got = Outputs(lay)
    V.dabplus_aus_table_dev(d_sf, sub, got.au, d_ret=d_ret, from_work=from_work)
    assert_same_buffers(got.host(), want, name)  # d_au; and nothing else is written
    assert np.array_equal(d_sf.cpu().numpy(), host)
    assert (model["status"] == AU_OK).any() and (model["status"] == AU_BAD_HEADER).any()
    assert (model["status"] == AU_RS_FAILED).any() == gated and (model["status"][[0, -1]] == AU_RS_FAILED).all() == gated


def test_table_without_a_dabplus_entry(V, torch_cuda):
    """nrec = npass = 0: both calls return OK with NULL d_rs_out, d_ret and d_au, launch nothing and write nothing"""
    sub = table(V, ONLY_PLAIN)
    lay = V.ensemble_layout(sub)
    assert int(lay["nrec"]) == 0 and int(lay["rs_bytes"]) == 0
    host = np.random.default_rng(8).integers(0, 256, int(lay["work_bytes"]), dtype=np.uint8)
    d_work = dev(host)
    got = Outputs(lay)
    V.rs_table_dev(d_work, None, None, sub)
    V.rs_table_dev(d_work, got.rs, got.ret, sub)
    for from_work in (False, True):
        V.dabplus_aus_table_dev(d_work, sub, None, d_ret=None, from_work=from_work)
        V.dabplus_aus_table_dev(d_work, sub, got.au, d_ret=got.ret, from_work=from_work)
    for buf, fill in zip(got.host(), (WORK_FILL, RS_FILL, RET_FILL, FLAG_FILL, FLAG_FILL)):
        assert (buf == fill).all()
    assert np.array_equal(d_work.cpu().numpy(), host)


# ---- 4. the chain on 64 small sub-channels --------------------------------------------------------------------------------

def chain_spec():
    """(RSDims or 0, framebits, phase, superframes or frames, profile) for 64 entries: RSDims 1 ... 3 at one or two
    superframes (one entry of RSDims 8), eight entries that are not DAB+ of 8 ... 192 bits - first and last among them -
    with 12 ... 33 frames; all phases distinct; one profile per frame length, shared by the entries of that length"""
    spec, lengths = [], []
    for k in range(64):
        phase = (k * 37) % 64  # 37 and 64 are coprime: every phase once
        if k % 9 == 0 or k == 63:
            fb, r, n = (8, 192, 64, 24, 192, 8, 120, 64, 8)[k // 9], 0, 12 + 3 * (k % 8)
        else:
            r = 8 if k == 40 else 1 + k % 3
            fb, n = 192 * r, 1 + (k // 3) % 2
        if fb not in lengths:
            lengths.append(fb)
        spec.append((r, fb, phase, n, lengths.index(fb)))
    return spec, lengths


MODES = ("3dB", "flip", "clean", "3dB", "junk", "3dB", "flip")


def build_chain(O):
    """tests/test_gpu_ensemble.py's build_ensemble for chain_spec(): CIF rows with every sub-channel at its phase and at
    CUs that leave unused columns between them, random bytes in a sub-channel's columns before and after its frames"""
    rng = np.random.default_rng(78)
    spec, lengths = chain_spec()
    e = types.SimpleNamespace(segs=[decodable_segments(rng, fb) for fb in lengths], punct=[], rows=[])
    pos, i = 1, 0
    for r, fb, phase, n, prof in spec:
        if r:
            _, sf = dabplus_superframes(rng, n, r)
            modes = [MODES[(i + s) % len(MODES)] for s in range(n)]
            sym, nframes, i = dabplus_symbols(O, rng, sf, r, modes), 5 * n, i + n
        else:
            frames = rng.integers(0, 256, (n, fb // 8), dtype=np.uint8)
            sym, nframes = channel(O, scramble(frames, fb), fb, rng, "3dB"), n
        punct = puncture(sym, e.segs[prof], fb)
        e.rows.append((fb, r, nframes, phase, CU * pos, prof, punct.shape[1]))
        e.punct.append(punct)
        pos += (punct.shape[1] + CU - 1) // CU + len(e.rows) % 2
    e.nframes = max(row[3] + row[2] for row in e.rows)
    width = CU * pos
    cif = rng.integers(0, 256, (e.nframes + 15, width), dtype=np.uint8)
    for row, punct in zip(e.rows, e.punct):
        cif[row[3]:row[3] + row[2] + 15, row[4]:row[4] + punct.shape[1]] = interleave(punct)
    e.nrows = e.nframes + 15 + 4
    e.first_row = e.nrows - 6  # the call's rows wrap
    e.ring = place_in_ring(cif, e.nrows, e.first_row, MSC_COL, MSC_COL + width + 3, rng, poison=POISON)
    return e


def test_chain_of_64_subchannels(V, O, torch_cuda):
    """more than 2 * TPB frames: three workgroups of vit_ens_desc_kernel, frame indices of vit_ens_post_kernel up to the
    last of 64 entries; against the calls per sub-channel and the oracle, as test_chain_equals_the_calls_per_subchannel"""
    e = build_chain(O)
    rows = e.rows
    sub = table(V, rows)
    lay = V.ensemble_layout(sub)
    total = sum(row[2] for row in rows)
    assert len(rows) == 64 and total > 2 * TPB and not rows[0][1] and not rows[63][1]
    assert len({row[3] for row in rows}) == 64 and int(lay["rows_needed"]) == e.nframes + 15
    shared = np.bincount([row[5] for row in rows])
    assert (shared >= 2).sum() >= 3 and len(e.segs) < 64 and len({str(s) for s in e.segs}) == len(e.segs)
    d_ring = dev_ring(e.ring)
    d_prof = torch.from_numpy(V.profiles_bytes(e.segs)).cuda()
    want = per_subchannel(V, e, d_ring, lay, rows).host()
    got = Outputs(lay)
    V.ensemble_dev(d_ring, e.first_row, MSC_COL, sub, d_prof, len(e.segs), got.work, got.rs, got.ret, got.fire, got.au)
    got = got.host()
    assert_same_buffers(got, want, "chain of 64")
    rets = []
    for k, (fb, r, nframes, _, _, prof, _) in enumerate(rows):
        work = scramble(O.decode_batch(fb, depuncture(e.punct[k], e.segs[prof], fb, 128), nthreads=8), fb)
        wo = int(lay["work_offset"][k])
        assert np.array_equal(got[0][wo:wo + work.size], work.reshape(-1)), k
        if r:
            ret, _ = O.rs_check_batch(work.reshape(nframes // 5, -1), r, np.full((nframes // 5, 110 * r), RS_FILL, np.uint8))
            ri = int(lay["rec_index"][k])
            assert got[2][ri:ri + ret.size].tolist() == ret.tolist(), k
            assert got[3][ri:ri + ret.size].tolist() == fire_ok_model(work.reshape(nframes // 5, -1)).tolist(), k
            rets += ret.tolist()
    assert len(rets) == int(lay["nrec"]) and any(v > 0 for v in rets) and any(v < 0 for v in rets) and rets.count(0) >= 8, rets
    au = got[4][:len(rets) * REC].view(AU_DTYPE)
    assert [int(s == AU_RS_FAILED) for s in au["status"]] == [int(v < 0) for v in rets]
