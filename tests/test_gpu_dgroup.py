"""GPU: vit_data_groups_dev against the model of tests/test_dgroup_host.py, byte for byte, with guard bytes around the
records, the summary and the data and in the alignment gaps between the groups' bytes; the inputs must stay as they were.
The long streams carry no real packet CRCs: the records say which packets are good, as vit_packets_dev would."""
import numpy as np
import pytest
import torch  # noqa: F401  (torch's runtime first, as when the whole suite is collected)

from test_dgroup_host import (DGROUP_SUM_DTYPE, DIRECTED, GUARD, PAD_DATA, PAD_DG, PAD_SUM, capacity_cases, dgroups_model,
                              expected_buffers, random_stream, same_buffers, synth_stream, total_bytes)
from test_gpu_dab import dev
from test_packet_host import PACKET_REC_DTYPE, PKT_DATA, PKT_PADDING, SLOT, build_framed_stream, packets_model

pytestmark = pytest.mark.gpu


def call_dev(V, torch, stream, rec, max_groups, capacity, with_data=True, byte_phase=0, data_phase=0):
    stream, rec = np.ascontiguousarray(stream, np.uint8), np.ascontiguousarray(rec)
    rec_bytes = np.frombuffer(rec.tobytes(), np.uint8).copy()
    d_bytes, d_rec = dev(stream, byte_phase), dev(rec_bytes)
    d_dg = torch.full((PAD_DG + 32 * max_groups + PAD_DG,), GUARD, dtype=torch.uint8, device="cuda")
    d_sum = torch.full((PAD_SUM + 32 + PAD_SUM,), GUARD, dtype=torch.uint8, device="cuda")
    d_data = torch.full((data_phase + PAD_DATA + capacity + PAD_DATA,), GUARD, dtype=torch.uint8, device="cuda")[data_phase:] if with_data else None
    V.data_groups_dev(d_bytes, d_rec, len(rec), d_dg[PAD_DG:], max_groups, d_sum[PAD_SUM:], d_data[PAD_DATA:] if with_data else None,
                      capacity)
    torch.cuda.synchronize()
    assert np.array_equal(d_bytes.cpu().numpy(), stream) and np.array_equal(d_rec.cpu().numpy(), rec_bytes)
    return d_dg.cpu().numpy(), d_sum.cpu().numpy(), d_data.cpu().numpy() if with_data else None


def check(V, torch, stream, rec, what, **kw):
    """everything written, with room to spare, and the records alone; returns the model's summary"""
    groups, summary = dgroups_model(stream, rec)
    ng, cap = len(groups) + 2, total_bytes(stream, rec) + 5
    same_buffers(call_dev(V, torch, stream, rec, ng, cap, **kw), expected_buffers(stream, rec, ng, cap), what)
    same_buffers(call_dev(V, torch, stream, rec, ng, 0, False, **kw), expected_buffers(stream, rec, ng, 0, False), what + ", records only")
    return summary


def placed_stream(rng, nslots, packets):
    """padding in every slot but the given one-slot data packets (slot, address, useful, cont, first, last)"""
    st = rng.integers(0, 256, SLOT * nslots, dtype=np.uint8)
    rec = np.zeros(nslots, PACKET_REC_DTYPE)
    rec["kind"], rec["crc_ok"], rec["nslots"] = PKT_PADDING, 1, 1
    st[0::SLOT], st[1::SLOT] = 0, 0
    for slot, a, useful, cont, first, last in packets:
        st[SLOT * slot:SLOT * slot + 3] = (cont << 4 | first << 3 | last << 2 | a >> 8, a & 255, useful)
        rec[slot] = (PKT_DATA, 1, 1, cont | last << 2 | first << 3, a, useful, 0)
    return st, rec


@pytest.mark.parametrize("name", sorted(DIRECTED))
def test_directed_streams(V, torch_cuda, name):
    check(V, torch_cuda, *DIRECTED[name], name)


def geometry_sizes(V):
    return sorted({1, 63, 64, 65} | {v + d for v in V.DGROUP_GEOMETRY.values() for d in (-1, 0, 1)})


def test_window_lengths_at_every_partition_edge(V, torch_cuda):
    rng = np.random.default_rng(21)
    sizes = geometry_sizes(V)
    assert {1023, 1024, 1025, 4095, 4097, 16383, 16384, 16385} <= set(sizes)
    ngroups = 0
    for n in sizes:
        stream, rec = synth_stream(rng, n)
        ngroups += check(V, torch_cuda, stream, rec, "%d slots" % n)["ngroups"]
    assert ngroups > 1000


@pytest.mark.parametrize("which", ["link_tile", "link_chunk", "number_block", "gather_step"])
def test_runs_across_a_partition_boundary(V, torch_cuda, which):
    """at the boundary B: a group whose packets straddle it, a run that breaks exactly on it, a run that is open across two
    whole parts and closes behind them, and one that stays open"""
    rng = np.random.default_rng(22)
    B = V.DGROUP_GEOMETRY[which]
    T = B if which != "link_chunk" else V.DGROUP_GEOMETRY["link_tile"]
    pk = [(B - 5, 10, 7, 3, 1, 0), (B - 1, 10, 19, 0, 0, 0), (B + 2, 10, 5, 1, 0, 1),
          (B - 4, 11, 9, 0, 1, 0), (B - 2, 11, 9, 1, 0, 0), (B, 11, 9, 3, 0, 0), (B + 3, 11, 9, 0, 0, 1),
          (B - 3, 12, 11, 2, 1, 0), (B + 2 * T + 3, 12, 13, 3, 0, 1),
          (B + 1, 13, 4, 0, 1, 0), (B + 2 * T + 1, 13, 4, 1, 0, 0)]
    stream, rec = placed_stream(rng, B + 2 * T + 6, pk)
    s = check(V, torch_cuda, stream, rec, which)
    assert (s["ngroups"], s["n_used"], s["n_dropped"], s["open_from"]) == (2, 5, 4, B + 1)


def test_run_open_across_two_whole_chunks(V, torch_cuda):
    rng = np.random.default_rng(23)
    C = V.DGROUP_GEOMETRY["link_chunk"]
    pk = [(C - 1, 500, 19, 1, 1, 0), (3 * C, 500, 19, 2, 0, 0), (3 * C + 1, 500, 2, 3, 0, 1), (5, 501, 3, 0, 1, 0), (3 * C + 2, 501, 3, 1, 0, 0)]
    stream, rec = placed_stream(rng, 3 * C + 3, pk)
    s = check(V, torch_cuda, stream, rec, "two whole chunks")
    assert (s["ngroups"], s["n_used"], s["open_from"]) == (1, 3, 5)


def test_groups_around_a_gather_step(V, torch_cuda):
    """groups of one packet fewer than a wavefront takes per step, as many, and one more, back to back and interleaved"""
    rng = np.random.default_rng(24)
    G = V.DGROUP_GEOMETRY["gather_step"]
    pk, slot = [], 3
    for n in (G - 1, G, G + 1, 2 * G + 1):
        for k in range(n):
            pk.append((slot, 700, int(rng.integers(0, 20)), k & 3, int(k == 0), int(k == n - 1)))
            slot += 1
    for k in range(G + 1):      # every third slot: the group spans more than three steps
        pk.append((slot + 3 * k, 701, int(rng.integers(0, 20)), k & 3, int(k == 0), int(k == G)))
    stream, rec = placed_stream(rng, slot + 3 * G + 9, pk)
    assert check(V, torch_cuda, stream, rec, "gather steps")["ngroups"] == 5


def test_every_data_address_present(V, torch_cuda):
    rng = np.random.default_rng(25)
    addrs = rng.permutation(np.arange(1, 1022))
    stream, rec = placed_stream(rng, 1021, [(i, int(a), int(rng.integers(0, 20)), 0, 1, 1) for i, a in enumerate(addrs)])
    assert check(V, torch_cuda, stream, rec, "1021 addresses")["ngroups"] == 1021


def test_byte_phases_of_the_stream_and_the_data(V, torch_cuda):
    rng = np.random.default_rng(26)
    stream, rec = synth_stream(rng, 200)
    ng, cap = dgroups_model(stream, rec)[1]["ngroups"], total_bytes(stream, rec)
    want = expected_buffers(stream, rec, ng, cap)
    for phase in range(16):
        same_buffers(call_dev(V, torch_cuda, stream, rec, ng, cap, byte_phase=phase, data_phase=phase % 4), want, "phase %d" % phase)


def test_every_length_mod_16(V, torch_cuda):
    rng = np.random.default_rng(27)
    lengths = [int(x) for x in rng.permutation(np.arange(0, 39))]
    pk = []
    for k, L in enumerate(lengths):     # two packets each
        a = L // 2
        pk += [(2 * k, 30, a, 0, 1, 0), (2 * k + 1, 30, L - a, 1, 0, 1)]
    stream, rec = placed_stream(rng, 2 * len(lengths), pk)
    groups = dgroups_model(stream, rec)[0]
    assert {len(g["D"]) % 16 for g in groups} == set(range(16)) and [len(g["D"]) for g in groups] == lengths
    for data_phase in range(4):
        cap = total_bytes(stream, rec)
        same_buffers(call_dev(V, torch_cuda, stream, rec, len(groups), cap, data_phase=data_phase),
                     expected_buffers(stream, rec, len(groups), cap), "data phase %d" % data_phase)


def test_capacity_edges(V, torch_cuda):
    stream, rec = DIRECTED["groups_2_3_5_9"]
    for mg, cap, wd in capacity_cases(stream, rec):
        same_buffers(call_dev(V, torch_cuda, stream, rec, mg, cap, wd), expected_buffers(stream, rec, mg, cap, wd),
                     "max_groups %d capacity %d" % (mg, cap))


def test_chain_from_a_framed_stream_with_fec(V, torch_cuda):
    """packets_dev, then data_groups_dev on its records, against the model applied to the bytes"""
    rng = np.random.default_rng(28)
    stream = build_framed_stream(rng, 2, 5, 216, 8)
    rec = packets_model(stream, 192)
    groups, summary = dgroups_model(stream, rec)
    assert len(groups) >= 5 and summary["n_dropped"] >= 5
    n, cap = len(rec), total_bytes(stream, rec)
    d_bytes = dev(stream, 3)
    d_rec = torch_cuda.full((8 * n,), 0xEE, dtype=torch_cuda.uint8, device="cuda")
    d_dg = torch_cuda.full((PAD_DG + 32 * len(groups) + PAD_DG,), GUARD, dtype=torch_cuda.uint8, device="cuda")
    d_sum = torch_cuda.full((PAD_SUM + 32 + PAD_SUM,), GUARD, dtype=torch_cuda.uint8, device="cuda")
    d_data = torch_cuda.full((PAD_DATA + cap + PAD_DATA,), GUARD, dtype=torch_cuda.uint8, device="cuda")
    V.packets_dev(d_bytes, 192, n // 8, d_rec)
    V.data_groups_dev(d_bytes, d_rec, n, d_dg[PAD_DG:], len(groups), d_sum[PAD_SUM:], d_data[PAD_DATA:], cap)
    torch_cuda.cuda.synchronize()
    assert d_rec.cpu().numpy().tobytes() == rec.tobytes()
    same_buffers((d_dg.cpu().numpy(), d_sum.cpu().numpy(), d_data.cpu().numpy()), expected_buffers(stream, rec, len(groups), cap), "chain")


def test_random_stream_twice(V, torch_cuda):
    stream, rec = random_stream()
    groups, summary = dgroups_model(stream, rec)
    assert len(groups) >= 200 and summary["n_dropped"] >= 50, "vacuous: %d groups, %d dropped" % (len(groups), summary["n_dropped"])
    cap = total_bytes(stream, rec)
    one = call_dev(V, torch_cuda, stream, rec, len(groups), cap)
    two = call_dev(V, torch_cuda, stream, rec, len(groups), cap)
    same_buffers(one, expected_buffers(stream, rec, len(groups), cap), "random stream")
    same_buffers(two, one, "second run")


def test_argument_errors(V, torch_cuda):
    L = V.lib()
    stream, rec = DIRECTED["one_packet"]
    d_bytes, d_rec = dev(stream), dev(np.frombuffer(rec.tobytes(), np.uint8).copy())
    out = torch_cuda.full((256,), GUARD, dtype=torch_cuda.uint8, device="cuda")
    s, r, d, m, x = d_bytes.data_ptr(), d_rec.data_ptr(), out.data_ptr(), out.data_ptr() + 64, out.data_ptr() + 128
    for args in ((None, r, 1, d, 1, m, x, 64), (s, None, 1, d, 1, m, x, 64), (s, r, 1, d, 1, None, x, 64), (s, r, 1, None, 1, m, x, 64),
                 (s, r + 2, 1, d, 1, m, x, 64), (s, r, 1, d + 1, 1, m, x, 64), (s, r, 1, d, 1, m + 2, x, 64),
                 (s, r, -1, d, 1, m, x, 64), (s, r, (1 << 24) + 1, d, 1, m, x, 64), (s, r, 1, d, 1, m, None, 64)):
        assert L.vit_data_groups_dev(*args, None) == 1 and "vit_data_groups_dev" in V.last_error()
    assert L.vit_data_groups_dev(s, r, 0, d, 1, m, x, 64, None) == 0
    torch_cuda.cuda.synchronize()
    assert bool((out == GUARD).all())
    assert L.vit_data_groups_dev(s, r, 1, None, 0, m, None, 0, None) == 0
    torch_cuda.cuda.synchronize()
    got = np.frombuffer(out.cpu().numpy()[64:96].tobytes(), DGROUP_SUM_DTYPE)[0]
    assert (got["ngroups"], got["nwritten"], got["data_bytes"], got["open_from"], got["n_used"]) == (1, 0, 16, 1, 1)
