"""GPU: a whole ensemble in one table-driven chain (vit_rs_table_dev, vit_dabplus_aus_table_dev, vit_ensemble_dev)
against the existing calls run per sub-channel on the same bytes, the oracle and the models of the host tests.
Everything is compared byte for byte and word for word: output buffers start as a sentinel and are compared WHOLE - the
gaps between the sub-channels' blocks and the slack behind the end included.

The RS table kernel gives every workgroup pass to ONE sub-channel (no packing of different widths into a pass), so the
mixed-wave case of the cooperative Chien search does not exist here and has no test."""
import os
import sys
import types

import numpy as np
import pytest
import torch  # noqa: F401  (torch's runtime first, as when the whole suite is collected)

from test_au_host import AU_BAD_HEADER, AU_DTYPE, AU_OK, AU_RS_FAILED, au_table_model, same
from test_dab_host import fire_ok_model, scramble
from test_gpu_au import random_batch
from test_gpu_dab import channel, dabplus_superframes, dabplus_symbols, decodable_segments, dev
from test_punct_host import depuncture, puncture
from test_ti_host import CU, interleave, place_in_ring

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import reffix  # noqa: E402
import rsdirect as D  # noqa: E402

pytestmark = pytest.mark.gpu

REC = AU_DTYPE.itemsize  # 20
SLACK = 48
WORK_FILL, RS_FILL, RET_FILL, FLAG_FILL = 0xEE, reffix.RS_SENTINEL, 0x7777, 0xEE
POISON = 0xA5


def table(V, rows):
    """(framebits, RSDims, nframes[, phase, col, profile, nsym]) per entry -> ENS_SUBCH_DTYPE array"""
    sub = np.zeros(len(rows), V.ENS_SUBCH_DTYPE)
    for k, r in enumerate(rows):
        r = tuple(r) + (0, 0, 0, 0)[len(r) - 3:]
        sub[k] = (r[4], r[5], r[0], r[1], r[3], r[2], r[6], 0)
    return sub


def dabplus_rows(dims_nsf):
    return [(192 * r, r, 5 * n) for r, n in dims_nsf]


class Outputs:
    """the five output buffers of a table in its layout, sentinel-filled, SLACK bytes (records) behind each end"""

    def __init__(self, lay, rs_offset=0):
        self.nrec = int(lay["nrec"])
        full = lambda n, v, dt=torch.uint8: torch.full((n,), v, dtype=dt, device="cuda")  # noqa: E731
        self.work = full(int(lay["work_bytes"]) + SLACK, WORK_FILL)
        self._rs = full(rs_offset + int(lay["rs_bytes"]) + SLACK, RS_FILL)
        self.rs = self._rs[rs_offset:]
        self.ret = full(self.nrec + 4, RET_FILL, torch.int32)
        self.fire = full(self.nrec + 4, FLAG_FILL)
        self.au = full((self.nrec + 2) * REC, FLAG_FILL)

    def host(self):
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (self.work, self._rs, self.ret, self.fire, self.au)]


NAMES = ("d_work", "d_rs_out", "d_ret", "d_fire_ok", "d_au")


def assert_same_buffers(got, want, what, names=NAMES):
    for name, g, w in zip(NAMES, got, want):
        if name in names:
            bad = np.flatnonzero(g != w)
            assert bad.size == 0, "%s: %s differs at %d places, first %s" % (what, name, bad.size, bad[:8])


# ---- 1. table RS against the uniform call -------------------------------------------------------------------------------

RS_TABLE = [(1, 3), (3, 1), (7, 2), (8, 37), (24, 2), (48, 6)]  # (RSDims, superframes)
# (sub-channel, superframe, column) -> an uncorrectable class: the first, a middle and the last column of a superframe, in
# sub-channels of one pass (3, 24) and of two (8: 32 superframes per pass; 48: 5 per pass)
RS_FAILURES = {(1, 0, 1): "deg2_noroot", (3, 5, 0): "nosplit_3", (3, 20, 3): "deg6_bad", (3, 36, 7): "deg2_noroot",
               (4, 1, 23): "nosplit_3", (5, 2, 0): "deg6_bad", (5, 4, 24): "deg2_noroot", (5, 5, 47): "nosplit_3"}
# clean superframes of ANOTHER sub-channel directly before and after the uncorrectable (1, 0): records 2 and 4
RS_CLEAN = {(0, 2), (2, 0)}
RS_MIX = ("clean", "single", "real_1", "real_2", "real_3", "real_4", "real_5", "clean", "clean", "real_2", "single")


def rs_blocks(pool):
    """the RS input block (nsf, 120 * rsdims) of every sub-channel of RS_TABLE from rsdirect's columns: clean ones, 1 ... 5
    errors, and the failures above"""
    blocks = []
    for k, (r, nsf) in enumerate(RS_TABLE):
        idx = np.zeros((nsf, r), np.int64)
        for s in range(nsf):
            for j in range(r):
                label = RS_FAILURES.get((k, s, j)) or ("clean" if (k, s) in RS_CLEAN else RS_MIX[(3 * s + j + k + 1) % len(RS_MIX)])
                idx[s, j] = pool.take(label)
        blocks.append(D.superframes(pool, idx))
    return blocks


def in_work_layout(lay, blocks, fill=0x3C):
    host = np.full(int(lay["work_bytes"]), fill, np.uint8)
    for k, b in enumerate(blocks):
        o = int(lay["work_offset"][k])
        host[o:o + b.size] = b.reshape(-1)
    return host


@pytest.mark.parametrize("offset", [0, 1])
def test_rs_table_equals_the_uniform_call(V, O, torch_cuda, offset):
    """offset 0: the 8-byte register prefetch, 16-byte output pieces; offset 1 (input and output): the fall-back copies"""
    sub = table(V, dabplus_rows(RS_TABLE))
    lay = V.ensemble_layout(sub)
    assert [int(x) % 16 for x in lay["work_offset"][:6]] == [0] * 6 and int(lay["rs_offset"][1]) == 336  # behind 330 bytes
    blocks = rs_blocks(D.Pool())
    d_work = dev(in_work_layout(lay, blocks), offset)
    got, want = Outputs(lay, offset), Outputs(lay, offset)
    V.rs_table_dev(d_work, got.rs, got.ret, sub)
    oracle_ret = []
    for k, (r, nsf) in enumerate(RS_TABLE):
        wo, ro, ri = (int(lay[n][k]) for n in ("work_offset", "rs_offset", "rec_index"))
        V.rs_batch_dev(d_work[wo:], want.rs[ro:], want.ret[ri:], r, nsf)
        ret, out = O.rs_check_batch(blocks[k], r, np.full((nsf, 110 * r), RS_FILL, np.uint8))
        oracle_ret += ret.tolist()
        torch.cuda.synchronize()
        assert np.array_equal(want.rs[ro:ro + out.size].cpu().numpy(), out.reshape(-1)), k
    got, want = got.host(), want.host()
    assert_same_buffers(got, want, "rs table", ("d_rs_out", "d_ret"))
    ret = got[2][:len(oracle_ret)].tolist()
    assert ret == oracle_ret and (got[2][len(oracle_ret):] == RET_FILL).all()
    first = [int(x) for x in lay["rec_index"][:6]]
    failed = sorted(first[k] + s for k, s, _ in RS_FAILURES)
    assert [i for i, v in enumerate(ret) if v < 0] == failed
    assert ret[2] == 0 and ret[4] == 0 and ret[3] == -1  # clean neighbours of another sub-channel around a failure
    assert max(ret) >= 5 * 3 and sum(v > 0 for v in ret) >= 30


# ---- 2. table access units against the uniform call and the model -------------------------------------------------------

@pytest.fixture(scope="module")
def au_case():
    rng = np.random.default_rng(2024)
    sfs = [random_batch(rng, r, nsf) for r, nsf in RS_TABLE]
    nrec = sum(n for _, n in RS_TABLE)
    ret = rng.integers(0, 4, nrec).astype(np.int32)
    ret[[1, 3, 9, nrec - 1]] = -1
    return sfs, ret


def au_reference(V, lay, sfs, d_sf, from_work, d_ret, ret):
    """records of vit_dabplus_aus_dev per sub-channel on the same device bytes, checked against the model"""
    want = Outputs(lay)
    model = []
    for k, (r, nsf) in enumerate(RS_TABLE):
        o, ri = int(lay["work_offset" if from_work else "rs_offset"][k]), int(lay["rec_index"][k])
        V.dabplus_aus_dev(d_sf[o:], r, nsf, want.au[ri * REC:], d_ret=None if d_ret is None else d_ret[ri:],
                          sf_stride=(120 if from_work else 110) * r)
        model.append(au_table_model(sfs[k], r, None if ret is None else ret[ri:ri + nsf]))
    want = want.host()
    model = np.concatenate(model)
    assert same(want[4][:model.size * REC].view(AU_DTYPE), model)
    return want, model


@pytest.mark.parametrize("from_work", [False, True])
@pytest.mark.parametrize("gated", [False, True])
def test_au_table_equals_the_uniform_call(V, torch_cuda, au_case, from_work, gated):
    sfs, ret = au_case
    sub = table(V, dabplus_rows(RS_TABLE))
    lay = V.ensemble_layout(sub)
    if from_work:  # the superframe before RS: the first 110 rows of each 120-row block
        host = in_work_layout(lay, [np.concatenate([s, np.full((s.shape[0], s.shape[1] // 11), 0x77, np.uint8)], axis=1)
                                    for s in sfs])
    else:
        host = np.full(int(lay["rs_bytes"]), 0x3C, np.uint8)
        for k, s in enumerate(sfs):
            o = int(lay["rs_offset"][k])
            host[o:o + s.size] = s.reshape(-1)
    d_sf = dev(host, 1 if from_work else 0)
    d_ret = torch.from_numpy(ret).cuda() if gated else None
    want, model = au_reference(V, lay, sfs, d_sf, from_work, d_ret, ret if gated else None)
    got = Outputs(lay)
    V.dabplus_aus_table_dev(d_sf, sub, got.au, d_ret=d_ret, from_work=from_work)
    assert_same_buffers(got.host(), want, "au table", ("d_au",))
    assert np.array_equal(d_sf.cpu().numpy(), host)
    assert set(model["num_aus"][model["status"] == AU_OK].tolist()) == {2, 3, 4, 6}
    assert (model["status"] == AU_BAD_HEADER).any() and (model["status"] == AU_RS_FAILED).any() == gated


# ---- 4. the chain ---------------------------------------------------------------------------------------------------

# (RSDims or 0, framebits, phase, superframes or frames, channel modes per superframe)
ENSEMBLE = [(1, 192, 0, 2, ["3dB", "flip"]), (3, 576, 1, 1, ["junk"]), (0, 1536, 5, 3, None), (8, 1536, 2, 2, ["clean", "3dB"]),
            (12, 2304, 3, 1, ["flip"]), (0, 8, 9, 1, None), (24, 4608, 4, 1, ["3dB"]), (48, 9216, 7, 1, ["flip"])]
MSC_COL = 5


def build_ensemble(O):
    """the ensemble of ENSEMBLE as CIF rows: every sub-channel with a profile of its own, at CUs that leave unused columns
    between them; the rows outside a sub-channel's own frames hold random bytes (its stream before and after)"""
    rng = np.random.default_rng(77)
    e = types.SimpleNamespace(segs=[], punct=[], rows=[])
    pos = 1
    for r, fb, phase, n, modes in ENSEMBLE:
        segs = decodable_segments(rng, fb)
        if r:
            _, sf = dabplus_superframes(rng, n, r)
            sym, nframes = dabplus_symbols(O, rng, sf, r, modes), 5 * n
        else:
            frames = rng.integers(0, 256, (n, fb // 8), dtype=np.uint8)
            sym, nframes = channel(O, scramble(frames, fb), fb, rng, "3dB"), n
        punct = puncture(sym, segs, fb)
        e.rows.append((fb, r, nframes, phase, CU * pos, len(e.segs), punct.shape[1]))
        e.segs.append(segs)
        e.punct.append(punct)
        pos += (punct.shape[1] + CU - 1) // CU + 1 + len(e.segs) % 3
    e.nframes = max(row[3] + row[2] for row in e.rows)
    width = CU * pos
    cif = rng.integers(0, 256, (e.nframes + 15, width), dtype=np.uint8)
    for row, punct in zip(e.rows, e.punct):
        cif[row[3]:row[3] + row[2] + 15, row[4]:row[4] + punct.shape[1]] = interleave(punct)
    e.nrows = e.nframes + 15 + 4
    e.first_row = e.nrows - 6  # the call's rows wrap
    e.ring = place_in_ring(cif, e.nrows, e.first_row, MSC_COL, MSC_COL + width + 3, rng, poison=POISON)
    return e


@pytest.fixture(scope="module")
def ens(O):
    return build_ensemble(O)


def dev_ring(ring):
    flat = np.ascontiguousarray(ring).reshape(-1)
    buf = torch.full((1 + flat.size + 64,), POISON, dtype=torch.uint8, device="cuda")
    buf[1:1 + flat.size] = torch.from_numpy(flat).cuda()
    return buf[1:1 + flat.size].view(ring.shape)


def per_subchannel(V, e, d_ring, lay, rows, only=None):
    """the existing calls, one sub-channel at a time, into sentinel-filled buffers of the table's layout"""
    want = Outputs(lay)
    for k, (fb, r, nframes, phase, col, prof, _) in enumerate(rows):
        if only is not None and k not in only:
            continue
        wo, ro, ri = (int(lay[n][k]) for n in ("work_offset", "rs_offset", "rec_index"))
        first = (e.first_row + phase) % e.nrows
        if r:
            V.dabplus_ti_superframes_dev(d_ring, first, MSC_COL + col, e.segs[prof], want.work[wo:], want.rs[ro:], want.ret[ri:],
                                         r, nframes // 5, d_fire_ok=want.fire[ri:])
            V.dabplus_aus_dev(want.rs[ro:], r, nframes // 5, want.au[ri * REC:], d_ret=want.ret[ri:])
        else:
            V.decode_punctured_ti_dev(d_ring, first, MSC_COL + col, want.work[wo:], fb, nframes, e.segs[prof])
            V.energy_dispersal_dev(want.work[wo:], fb, nframes)
    return want


@pytest.mark.parametrize("ge", [False, True])
def test_chain_equals_the_calls_per_subchannel(V, O, torch_cuda, ens, ge):
    e = ens
    sub = table(V, e.rows)
    lay = V.ensemble_layout(sub)
    assert int(lay["rows_needed"]) == e.nframes + 15 == e.nrows - 4 and len({str(s) for s in e.segs}) == len(e.segs)
    d_ring = dev_ring(e.ring)
    d_prof = torch.from_numpy(V.profiles_bytes(e.segs)).cuda()
    old = V.set_renorm_ge(ge)
    try:
        want = per_subchannel(V, e, d_ring, lay, e.rows).host()
        got, part = Outputs(lay), Outputs(lay)
        V.ensemble_dev(d_ring, e.first_row, MSC_COL, sub, d_prof, len(e.segs), got.work, got.rs, got.ret, got.fire, got.au)
        V.ensemble_dev(d_ring, e.first_row, MSC_COL, sub, d_prof, len(e.segs), part.work, part.rs, part.ret)  # no flags, no AUs
        got, part = got.host(), part.host()
    finally:
        V.set_renorm_ge(old)
    assert_same_buffers(got, want, "chain")
    assert_same_buffers(part, want, "chain without d_fire_ok and d_au", ("d_work", "d_rs_out", "d_ret"))
    assert (part[3] == FLAG_FILL).all() and (part[4] == FLAG_FILL).all()
    # the oracle on the same symbols: d_work, the return values, the fire flags
    rets = []
    for k, (fb, r, nframes, _, _, prof, _) in enumerate(e.rows):
        work = scramble(O.decode_batch(fb, depuncture(e.punct[k], e.segs[prof], fb, 128), ge=ge, nthreads=8), fb)
        wo = int(lay["work_offset"][k])
        assert np.array_equal(got[0][wo:wo + work.size], work.reshape(-1)), k
        if r:
            ret, _ = O.rs_check_batch(work.reshape(nframes // 5, -1), r, np.full((nframes // 5, 110 * r), RS_FILL, np.uint8))
            ri = int(lay["rec_index"][k])
            assert got[2][ri:ri + ret.size].tolist() == ret.tolist(), k
            assert got[3][ri:ri + ret.size].tolist() == fire_ok_model(work.reshape(nframes // 5, -1)).tolist(), k
            rets += ret.tolist()
    assert any(v > 0 for v in rets) and any(v < 0 for v in rets) and rets[3] == 0, rets  # corrected, given up, clean
    au = got[4][:len(rets) * REC].view(AU_DTYPE)
    assert [int(s == AU_RS_FAILED) for s in au["status"]] == [int(v < 0) for v in rets]


def test_chain_ring_one_row_short(V, torch_cuda, ens):
    e = ens
    sub = table(V, e.rows)
    lay = V.ensemble_layout(sub)
    d_ring = dev_ring(e.ring)[:int(lay["rows_needed"]) - 1]
    d_prof = torch.from_numpy(V.profiles_bytes(e.segs)).cuda()
    got = Outputs(lay)
    with pytest.raises(V.ViterbiError, match="rows"):
        V.ensemble_dev(d_ring, 0, MSC_COL, sub, d_prof, len(e.segs), got.work, got.rs, got.ret, got.fire, got.au)
    for buf, fill in zip(got.host(), (WORK_FILL, RS_FILL, RET_FILL, FLAG_FILL, FLAG_FILL)):
        assert (buf == fill).all()


def test_chain_argument_rules(V, torch_cuda, ens):
    """checked on the host before anything is launched: columns outside a row, a column that is no multiple of 16, a
    profile index beyond the table, a table that breaks a rule of the layout"""
    e = ens
    lay = V.ensemble_layout(table(V, e.rows))
    d_ring = dev_ring(e.ring)
    d_prof = torch.from_numpy(V.profiles_bytes(e.segs)).cuda()
    got = Outputs(lay)

    def call(rows, nprof=len(e.segs), msc_col=MSC_COL):
        with pytest.raises(V.ViterbiError, match="bad arguments"):
            V.ensemble_dev(d_ring, e.first_row, msc_col, table(V, rows), d_prof, nprof, got.work, got.rs, got.ret, got.fire, got.au)

    change = lambda k, **kw: [tuple(kw.get(n, v) for n, v in zip(("fb", "r", "nf", "phase", "col", "prof", "nsym"), row))  # noqa: E731
                              if i == k else row for i, row in enumerate(e.rows)]
    room = e.ring.shape[1] - (MSC_COL + e.rows[7][4] + e.rows[7][6])  # columns behind the last sub-channel's end
    call(e.rows, msc_col=MSC_COL + room + 1)
    call(change(7, nsym=e.rows[7][6] + room + 1))
    call(e.rows, msc_col=(1 << 64) - 64)              # wraps
    call(change(2, col=e.rows[2][4] + 8))
    call(e.rows, nprof=len(e.segs) - 1)
    call(change(4, prof=len(e.segs)))
    call(change(4, nf=6))
    for buf, fill in zip(got.host(), (WORK_FILL, RS_FILL, RET_FILL, FLAG_FILL, FLAG_FILL)):
        assert (buf == fill).all()


# ---- 5. one entry; an invalid profile on the device -----------------------------------------------------------------------

def test_one_entry_equals_the_uniform_chain(V, torch_cuda, ens):
    e = ens
    rows = [e.rows[3]]  # RSDims 8, phase 2, two superframes
    sub = table(V, rows)
    lay = V.ensemble_layout(sub)
    d_ring = dev_ring(e.ring)
    d_prof = torch.from_numpy(V.profiles_bytes(e.segs)).cuda()
    want = per_subchannel(V, e, d_ring, lay, rows).host()
    got = Outputs(lay)
    V.ensemble_dev(d_ring, e.first_row, MSC_COL, sub, d_prof, len(e.segs), got.work, got.rs, got.ret, got.fire, got.au)
    assert_same_buffers(got.host(), want, "one entry")


def test_invalid_profile_contents_skip_exactly_that_subchannel(V, torch_cuda, ens):
    """sub-channel 4's profile on the device covers one step too few: its d_work bytes stay at the sentinel, the later
    stages run on them as they are, and every other sub-channel's outputs are what they were"""
    e = ens
    bad = 4
    sub = table(V, e.rows)
    lay = V.ensemble_layout(sub)
    d_ring = dev_ring(e.ring)
    fb, r, nframes = e.rows[bad][:3]
    profs = list(e.segs)
    profs[bad] = [(fb + 5, 0xFFFFFFFF)]
    d_prof = torch.from_numpy(V.profiles_bytes(profs)).cuda()
    want = per_subchannel(V, e, d_ring, lay, e.rows, only=set(range(len(e.rows))) - {bad})
    wo, ro, ri = (int(lay[n][bad]) for n in ("work_offset", "rs_offset", "rec_index"))
    nsf = nframes // 5
    V.rs_batch_dev(want.work[wo:], want.rs[ro:], want.ret[ri:], r, nsf)  # RS and the access units of the sentinel bytes
    V.dabplus_aus_dev(want.rs[ro:], r, nsf, want.au[ri * REC:], d_ret=want.ret[ri:])
    want.fire[ri:ri + nsf] = torch.from_numpy(fire_ok_model(np.full((nsf, 11), WORK_FILL, np.uint8))).cuda()
    want = want.host()
    assert (want[0][wo:wo + nframes * fb // 8] == WORK_FILL).all()
    got = Outputs(lay)
    V.ensemble_dev(d_ring, e.first_row, MSC_COL, sub, d_prof, len(profs), got.work, got.rs, got.ret, got.fire, got.au)
    assert_same_buffers(got.host(), want, "invalid profile")
