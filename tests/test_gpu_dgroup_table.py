"""GPU: data groups over a table of streams (vit_data_groups_table_dev) against the model of tests/test_dgroup_host.py applied
to every stream on its own, byte for byte.  Every output lies between guard bytes: in front of and behind the three
buffers, between the streams' blocks, in the 16-byte rounding gaps of d_data and behind each stream's nwritten records.
Between the streams' inputs lie bytes and records that would make groups if a kernel read them; the inputs must stay as
they were."""
import numpy as np
import pytest
import torch  # noqa: F401  (torch's runtime first, as when the whole suite is collected)

from test_dgroup_host import (DGROUP_SUM_DTYPE, DIRECTED, GUARD, PAD_DATA, PAD_DG, PAD_SUM, PKT_FIRST, PKT_LAST, capacity_cases,
                              dgroups_model, expected_buffers, random_stream, same_buffers, synth_stream)
from test_dgroup_table_host import layout_model
from test_gpu_dab import dev
from test_gpu_dgroup import call_dev, placed_stream
from test_gpu_packet import PAD, guarded
from test_gpu_packet_table import FEC_NONE, FEC_SEARCH, Stream, damage, filled, plant_headers, table_of
from test_packet_host import PACKET_REC_DTYPE, PKT_DATA, SLOT, build_framed_stream

pytestmark = pytest.mark.gpu

PREC = PACKET_REC_DTYPE.itemsize
FILL_BYTE = 0xC3
# what lies between the streams' records: a one-slot group of its own, if anything read it
TEMPTING = np.array([(PKT_DATA, 1, 1, PKT_FIRST | PKT_LAST, 5, 10, 0)], PACKET_REC_DTYPE)


class Entry:
    """a stream, its records and its limits; model_rec: the records the model is asked about, where they differ"""
    def __init__(self, stream, rec, max_groups=None, capacity=None, with_data=True, model_rec=None):
        self.stream, self.rec = np.ascontiguousarray(stream, np.uint8), np.ascontiguousarray(rec)
        self.model_rec = self.rec if model_rec is None else model_rec
        assert self.stream.size == SLOT * len(self.rec)
        if max_groups is None or capacity is None:     # everything written, with room to spare
            groups = dgroups_model(self.stream, self.model_rec)[0]
            max_groups = len(groups) + 2 if max_groups is None else max_groups
            capacity = (sum((len(g["D"]) + 15) // 16 * 16 for g in groups) + 5 if with_data else 0) if capacity is None else capacity
        self.max_groups, self.capacity, self.with_data = max_groups, capacity, with_data

    def want(self):
        return expected_buffers(self.stream, self.model_rec, self.max_groups, self.capacity, self.with_data)


def lay_out(V, entries, residues=None, adjacent=False, shared=None):
    """the streams and their record blocks with gaps between them (none if adjacent), stream k's bytes at an offset that is
    residues[k] mod 16; shared: {k: j} entry k reads entry j's bytes and records -> (table, bytes image, record image)"""
    shared = shared or {}
    bparts, rparts, offsets, rec_index, bcur, rcur = [], [], {}, {}, 0, 0
    for k, e in enumerate(entries):
        if k in shared:
            continue
        gap = 0 if adjacent and k else 8 + (0 if residues is None else (residues[k] - (bcur + 8)) % 16)
        rgap = 0 if adjacent and k else 1 + k % 3
        bparts += [np.full(gap, FILL_BYTE, np.uint8), e.stream]
        rparts += [np.repeat(TEMPTING, rgap), e.rec]
        offsets[k], rec_index[k] = bcur + gap, rcur + rgap
        bcur, rcur = bcur + gap + e.stream.size, rcur + rgap + len(e.rec)
    bparts.append(np.full(8, FILL_BYTE, np.uint8))
    rparts.append(np.repeat(TEMPTING, 2))
    tab = np.zeros(len(entries), V.DG_STREAM_DTYPE)
    for k, e in enumerate(entries):
        j = shared.get(k, k)
        tab[k] = (offsets[j], rec_index[j], len(e.rec), e.max_groups, e.capacity, 0 if e.with_data else 1)
    if residues is not None:
        assert [int(o) % 16 for o in tab["offset"]] == [r % 16 for r in residues]
    return tab, np.concatenate(bparts), np.concatenate(rparts)


def run_table(V, torch, tab, image, rec_image, byte_phase=0):
    """-> (records, summaries, data or None) as host arrays, guards included"""
    lay = V.data_groups_table_layout(tab)
    assert int(lay["bytes_end"]) <= image.size and int(lay["rec_end"]) <= len(rec_image)
    rec_bytes = np.frombuffer(rec_image.tobytes(), np.uint8).copy()
    d_bytes, d_rec = dev(image, byte_phase), dev(rec_bytes)
    d_dg = torch.full((PAD_DG + 32 * int(lay["ndg"]) + PAD_DG,), GUARD, dtype=torch.uint8, device="cuda")
    d_sum = torch.full((PAD_SUM + 32 * len(tab) + PAD_SUM,), GUARD, dtype=torch.uint8, device="cuda")
    with_data = bool((tab["records_only"] == 0).any())
    d_data = torch.full((PAD_DATA + int(lay["data_bytes"]) + PAD_DATA,), GUARD, dtype=torch.uint8, device="cuda") if with_data else None
    V.data_groups_table_dev(d_bytes, d_rec, tab, d_dg[PAD_DG:], d_sum[PAD_SUM:], d_data[PAD_DATA:] if with_data else None)
    torch.cuda.synchronize()
    assert np.array_equal(d_bytes.cpu().numpy(), image) and np.array_equal(d_rec.cpu().numpy(), rec_bytes), "the inputs changed"
    return d_dg.cpu().numpy(), d_sum.cpu().numpy(), d_data.cpu().numpy() if with_data else None


def expected(tab, entries):
    """what run_table must return: every stream's expected_buffers at its place, guard bytes everywhere else"""
    dg_index, data_offset, ndg, data_bytes, _, _ = layout_model(tab.tolist())
    dg = np.full(PAD_DG + 32 * ndg + PAD_DG, GUARD, np.uint8)
    sm = np.full(PAD_SUM + 32 * len(entries) + PAD_SUM, GUARD, np.uint8)
    data = np.full(PAD_DATA + data_bytes + PAD_DATA, GUARD, np.uint8) if any(e.with_data for e in entries) else None
    for k, e in enumerate(entries):
        w_dg, w_sm, w_data = e.want()
        dg[PAD_DG + 32 * dg_index[k]:PAD_DG + 32 * (dg_index[k] + e.max_groups)] = w_dg[PAD_DG:PAD_DG + 32 * e.max_groups]
        sm[PAD_SUM + 32 * k:PAD_SUM + 32 * (k + 1)] = w_sm[PAD_SUM:PAD_SUM + 32]
        if e.with_data:
            data[PAD_DATA + data_offset[k]:PAD_DATA + data_offset[k] + e.capacity] = w_data[PAD_DATA:PAD_DATA + e.capacity]
    return dg, sm, data


def summaries(got):
    return np.frombuffer(got[1][PAD_SUM:-PAD_SUM].tobytes(), DGROUP_SUM_DTYPE)


def check_table(V, torch, entries, what, byte_phase=0, **kw):
    tab, image, rec_image = lay_out(V, entries, **kw)
    got = run_table(V, torch, tab, image, rec_image, byte_phase)
    same_buffers(got, expected(tab, entries), what)
    return got


# ---- 1: partition edges, mixed in one table ---------------------------------------------------------------------------------
def test_partition_edges_mixed_in_one_table(V, torch_cuda):
    """one chunk and several, one block and several, in one table: the link totals pass runs for some streams only"""
    rng = np.random.default_rng(2601)
    G = V.DGROUP_GEOMETRY
    sizes = sorted({1, 63, 64, 65, 2 * G["link_chunk"] + 5} | {v + d for v in G.values() for d in (-1, 0, 1)})
    assert sizes == [1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385, 2 * 16384 + 5]
    sizes = [int(n) for n in rng.permutation(sizes + [2, 2 * G["number_block"] + 1])]     # sixteen streams: every residue mod 16
    assert sizes != sorted(sizes) and sizes != sorted(sizes, reverse=True)
    entries = [Entry(*synth_stream(rng, n), with_data=k % 5 != 3) for k, n in enumerate(sizes)]
    got = check_table(V, torch_cuda, entries, "partition edges", residues=[int(r) for r in rng.permutation(16)], byte_phase=3)
    assert int(summaries(got)["ngroups"].sum()) > 1000


# ---- 2: streams do not leak into each other ---------------------------------------------------------------------------------
@pytest.mark.parametrize("na", [100, 1024, 4096 + 300, 16384 + 9])
def test_streams_do_not_leak_into_each_other(V, torch_cuda, na):
    """A and B adjacent in d_bytes and d_rec; for na = 100 the boundary lies inside what would be one link tile and one block
    of the prefix sum if the slots were numbered through, for the others in later tiles, blocks and chunks"""
    rng = np.random.default_rng(2602)
    nb = 50
    X, Y, Z = 200, 300, 400
    a_stream, a_rec = placed_stream(rng, na, [(2, Z, 9, 0, 1, 0), (5, Z, 11, 1, 0, 1), (na - 3, X, 7, 1, 1, 0)])
    # A's last record claims a four-slot packet that is a group of its own: its end lies behind A, inside B's bytes
    a_rec[na - 1] = (PKT_DATA, 1, 4, PKT_FIRST | PKT_LAST, Y, 60, 0)
    a_model = a_rec.copy()
    a_model[na - 1]["crc_ok"] = 0       # the model has no window: unusable by the rule it does know
    b_stream, b_rec = placed_stream(rng, nb, [(0, X, 9, 2, 0, 0), (1, X, 5, 3, 0, 1), (3, Z, 4, 0, 1, 1), (6, Z, 8, 1, 1, 0), (8, Z, 3, 2, 0, 1)])
    # numbered through, X would run on from A into B and close there
    joined = dgroups_model(np.concatenate([a_stream, b_stream]), np.concatenate([a_model, b_rec]))[0]
    assert any(g["address"] == X and g["first_slot"] == na - 3 and g["last_slot"] == na + 1 for g in joined)
    entries = [Entry(a_stream, a_rec, model_rec=a_model), Entry(b_stream, b_rec)]
    got = check_table(V, torch_cuda, entries, "A then B, %d slots" % na, adjacent=True)
    sa, sb = summaries(got)
    assert (sa["ngroups"], sa["n_used"], sa["n_dropped"], sa["n_unusable"], sa["open_from"]) == (1, 2, 0, 1, na - 3)
    assert (sb["ngroups"], sb["n_used"], sb["n_dropped"], sb["n_unusable"], sb["open_from"]) == (2, 3, 2, 0, nb)
    # and with B in front of A in the table, still adjacent in memory
    tab, image, rec_image = lay_out(V, entries, adjacent=True)
    swapped = tab[::-1].copy()
    same_buffers(run_table(V, torch_cuda, swapped, image, rec_image), expected(swapped, entries[::-1]), "B then A")


# ---- 3: every data address present in two streams -----------------------------------------------------------------------------
def test_every_data_address_present_in_two_streams(V, torch_cuda):
    rng = np.random.default_rng(2603)
    entries = []
    for _ in range(2):
        addrs = rng.permutation(np.arange(1, 1022))
        entries.append(Entry(*placed_stream(rng, 1021, [(i, int(a), int(rng.integers(0, 20)), 0, 1, 1) for i, a in enumerate(addrs)])))
    assert not np.array_equal(entries[0].rec["address"], entries[1].rec["address"])
    entries.insert(1, Entry(*synth_stream(rng, 700, naddr=4)))
    got = check_table(V, torch_cuda, entries, "1021 addresses twice", residues=[5, 10, 15])
    assert summaries(got)["ngroups"].tolist()[::2] == [1021, 1021]


# ---- 4: per-stream limits ---------------------------------------------------------------------------------------------------
def test_per_stream_limits_in_one_table(V, torch_cuda):
    """capacity_cases, one per entry, all on the same two copies of the stream: a stream behind a cut-off one is unaffected
    and every nwritten is the stream's own"""
    stream, rec = DIRECTED["groups_2_3_5_9"]
    cases = capacity_cases(stream, rec)
    ng = len(dgroups_model(stream, rec)[0])
    assert {(0, True), (ng - 1, True), (ng, False), (0, False)} <= {(mg, wd) for mg, _, wd in cases}
    assert any(cap == 0 and wd and mg == ng for mg, cap, wd in cases)
    entries = [Entry(stream, rec, mg, cap, wd) for mg, cap, wd in cases]
    got = check_table(V, torch_cuda, entries, "limits", residues=[7] * len(cases), shared={k: k % 2 for k in range(2, len(cases))})
    nwritten = summaries(got)["nwritten"].tolist()
    want = [int(np.frombuffer(e.want()[1][PAD_SUM:PAD_SUM + 32].tobytes(), DGROUP_SUM_DTYPE)["nwritten"][0]) for e in entries]
    assert nwritten == want and 0 in nwritten and ng - 1 in nwritten and nwritten[2] == ng and len(set(nwritten)) >= 3
    assert (summaries(got)["ngroups"] == ng).all()


# ---- 5: table shapes --------------------------------------------------------------------------------------------------------
def test_64_one_slot_streams(V, torch_cuda):
    rng = np.random.default_rng(2605)
    entries = []
    for k in range(64):
        first, last = (k >> 0) & 1, (k >> 1) & 1
        pk = [] if k % 7 == 6 else [(0, int(rng.integers(1, 1022)), int(rng.integers(0, 20)), k & 3, first, last)]
        entries.append(Entry(*placed_stream(rng, 1, pk), max_groups=k % 3, capacity=(0, 1, 15, 16, 17, 40)[k % 6] if k % 4 else 0,
                             with_data=bool(k % 4)))
    got = check_table(V, torch_cuda, entries, "64 one-slot streams", residues=[(7 * k) % 16 for k in range(64)])
    s = summaries(got)
    assert 10 <= int(s["ngroups"].sum()) < 20 and 5 <= int(s["nwritten"].sum()) < int(s["ngroups"].sum())
    assert (s["open_from"] == 0).any() and (s["n_dropped"] == 1).any()


def test_table_of_one_stream_equals_the_per_stream_call(V, torch_cuda):
    rng = np.random.default_rng(2606)
    stream, rec = synth_stream(rng, 2 * V.DGROUP_GEOMETRY["link_chunk"] + 77)
    for with_data in (True, False):
        e = Entry(stream, rec, with_data=with_data)
        tab = np.array([(0, 0, len(rec), e.max_groups, e.capacity, 0 if with_data else 1)], V.DG_STREAM_DTYPE)
        dg, sm, data = run_table(V, torch_cuda, tab, stream, rec, byte_phase=5)
        if with_data:   # the layout rounds the stream's block up to 16: guard bytes behind the capacity, as behind the call's
            assert (data[PAD_DATA + e.capacity:] == GUARD).all()
            data = data[:PAD_DATA + e.capacity + PAD_DATA]
        got = (dg, sm, data)
        same_buffers(got, call_dev(V, torch_cuda, stream, rec, e.max_groups, e.capacity, with_data, byte_phase=5), "the per-stream call")
        same_buffers(got, e.want(), "the model")


# ---- 6: a random stream as three entries ------------------------------------------------------------------------------------
def test_random_stream_as_three_entries_twice(V, torch_cuda):
    stream, rec = random_stream()
    groups, summary = dgroups_model(stream, rec)
    assert len(groups) >= 200 and summary["n_dropped"] >= 50, "vacuous: %d groups, %d dropped" % (len(groups), summary["n_dropped"])
    entries = [Entry(stream, rec), Entry(stream, rec, with_data=False), Entry(stream, rec, max_groups=0)]
    tab, image, rec_image = lay_out(V, entries, residues=[1, 6, 11])
    one = run_table(V, torch_cuda, tab, image, rec_image)
    two = run_table(V, torch_cuda, tab, image, rec_image)
    same_buffers(one, expected(tab, entries), "random stream")
    same_buffers(two, one, "second run")


# ---- 7: behind vit_packet_table_dev -----------------------------------------------------------------------------------------
def test_chain_behind_the_packet_table(V, torch_cuda):
    """packet_table_dev, then data_groups_table_dev on its d_rec with rec_index from the packet layout, nothing copied to the
    host in between; against packets_model + dgroups_model on the corrected bytes"""
    torch = torch_cuda
    rng = np.random.default_rng(2607)
    st = damage(rng, plant_headers(build_framed_stream(rng, 2, 40, 256, 8), 40, 2), 40, [0, 1], 4)
    streams = [Stream(st, 192, FEC_SEARCH, planted=40), Stream(build_framed_stream(rng, 0, 0, 150, 3), 72, FEC_NONE)]
    ptab, image, streams, offsets = table_of(V, streams, residues=[3, 9])
    after = [s.model()[2] for s in streams]
    prec = [s.model()[4] for s in streams]
    assert streams[0].model()[1][0] == 40 and not np.array_equal(after[0], streams[0].data), "the FEC stage corrects bytes"
    entries = [Entry(a, r) for a, r in zip(after, prec)]
    for e in entries:
        groups, summary = dgroups_model(e.stream, e.rec)
        assert len(groups) >= 5 and summary["n_dropped"] >= 5
    play = V.packet_table_layout(ptab)
    tab = np.zeros(2, V.DG_STREAM_DTYPE)
    tab["offset"], tab["rec_index"] = ptab["offset"], play["rec_index"][:2]
    tab["nslots"], tab["max_groups"], tab["data_capacity"] = [s.nslots for s in streams], [e.max_groups for e in entries], [e.capacity for e in entries]
    lay = V.data_groups_table_layout(tab)
    assert int(lay["rec_end"]) == int(play["nrec"]) and int(lay["bytes_end"]) == int(play["bytes_end"])
    d, _ = guarded(image, 1)
    d_srec, d_fec, d_rec = filled(torch, 2 * 16), filled(torch, int(play["nfecrec"]) * 16), filled(torch, int(play["nrec"]) * PREC)
    d_dg = torch.full((PAD_DG + 32 * int(lay["ndg"]) + PAD_DG,), GUARD, dtype=torch.uint8, device="cuda")
    d_sum = torch.full((PAD_SUM + 64 + PAD_SUM,), GUARD, dtype=torch.uint8, device="cuda")
    d_data = torch.full((PAD_DATA + int(lay["data_bytes"]) + PAD_DATA,), GUARD, dtype=torch.uint8, device="cuda")
    V.packet_table_dev(d[PAD:], ptab, d_srec[16:], d_fec[16:], d_rec[16:])
    V.data_groups_table_dev(d[PAD:], d_rec[16:], tab, d_dg[PAD_DG:], d_sum[PAD_SUM:], d_data[PAD_DATA:])
    torch.cuda.synchronize()
    assert d_rec.cpu().numpy()[16:-16].tobytes() == np.concatenate(prec).tobytes()
    same_buffers((d_dg.cpu().numpy(), d_sum.cpu().numpy(), d_data.cpu().numpy()), expected(tab, entries), "chain")


# ---- 8: arguments -----------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(V, torch_cuda):
    torch = torch_cuda
    L = V.lib()
    stream, rec = DIRECTED["groups_2_3_5_9"]
    d_bytes, d_rec = dev(stream), dev(np.frombuffer(rec.tobytes(), np.uint8).copy())
    out = torch.full((1024,), GUARD, dtype=torch.uint8, device="cuda")
    s, r, d, m, x = d_bytes.data_ptr(), d_rec.data_ptr(), out.data_ptr(), out.data_ptr() + 512, out.data_ptr() + 640
    n = len(rec)
    good = np.array([(0, 0, n, 4, 100, 0), (0, 0, n, 4, 0, 1)], V.DG_STREAM_DTYPE)

    def table(*rows):
        return np.array(list(rows), V.DG_STREAM_DTYPE).reshape(-1)
    big = table(*[(0, 0, 1 << 24, 0, 0, 1)] * 4, (0, 0, 1, 0, 0, 1))
    calls = [(None, r, good, 2, d, m, x), (s, None, good, 2, d, m, x), (s, r, good, 2, d, None, x), (s, r, good, 2, None, m, x),
             (s, r, good, 2, d, m, None), (s, r + 2, good, 2, d, m, x), (s, r, good, 2, d + 1, m, x), (s, r, good, 2, d, m + 2, x),
             (s, r, good, 0, d, m, x), (s, r, np.repeat(good[:1], 65), 65, d, m, x), (s, r, None, 1, d, m, x),
             (s, r, table((0, 0, 0, 4, 100, 0)), 1, d, m, x), (s, r, table((0, 0, (1 << 24) + 1, 4, 100, 0)), 1, d, m, x),
             (s, r, table((0, 0, n, 4, 0, 2)), 1, d, m, x), (s, r, table((0, 0, n, 4, 16, 1)), 1, d, m, x),
             (s, r, table(((1 << 64) - 24, 0, n, 4, 100, 0)), 1, d, m, x), (s, r, table((0, (1 << 64) - 1, n, 4, 100, 0)), 1, d, m, x),
             (s, r, big, 5, d, m, x), (s, r, table((0, 0, n, 0xFFFFFFFF, 0, 0), (0, 0, n, 1, 0, 0), (0, 0, n, 1, 0, 0)), 3, d, m, x),
             (s, r, table((0, 0, n, 1, 0xFFFFFFF1, 0), (0, 0, n, 1, 0, 0)), 2, d, m, x)]
    for b, rr, t, nt, dg, sm, data in calls:
        rc = L.vit_data_groups_table_dev(b, rr, None if t is None else t.ctypes.data, nt, dg, sm, data, None)
        assert rc == 1 and "vit_data_groups_table_dev" in V.last_error(), V.last_error()
    assert "entry 1" in V.last_error()
    torch.cuda.synchronize()
    assert bool((out == GUARD).all())
    with pytest.raises(V.ViterbiError):
        V.data_groups_table_dev(d_bytes, d_rec, good, out, out[512:], None)
    # no room asked for anywhere: d_dg and d_data may be NULL, and the summaries are written
    none = table((0, 0, n, 0, 0, 0), (0, 0, n, 0, 0, 1))
    assert L.vit_data_groups_table_dev(s, r, none.ctypes.data, 2, None, m, None, None) == 0, V.last_error()
    torch.cuda.synchronize()
    got = np.frombuffer(out.cpu().numpy()[512:576].tobytes(), DGROUP_SUM_DTYPE)
    assert got["ngroups"].tolist() == [4, 4] and got["nwritten"].tolist() == [0, 0] and got["n_used"].tolist() == [19, 19]
    rest = out.cpu().numpy()
    assert (rest[:512] == GUARD).all() and (rest[576:] == GUARD).all()
