"""GPU: packet mode over a table of streams (vit_packet_table_dev) against the models and builders of
tests/test_packet_host.py and tests/test_packet_table_host.py, byte for byte: the stream records, the scores, the FEC
records, the packet records and the stream bytes; sentinel bytes between and around the streams and around every output,
FEC records past nfec untouched.  The one-stream tables and the mixed table are also compared with the three per-stream
device calls on a copy."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (torch's runtime first, as when the whole suite is collected)

from test_gpu_packet import PAD, guarded
from test_packet_host import (FEC_FRAME_BYTES, FEC_REC_DTYPE, FEC_SLOTS, PACKET_REC_DTYPE, PKT_FEC, SLOT, build_framed_stream,
                              build_stream, fec_hdr, fec_stream_model, packets_model, random_damaged_frame, same, sync_model)
from test_packet_table_host import FEC_NONE, FEC_PHASE, FEC_SEARCH, NO_PHASE, fec_count, layout_model, pick_model, stream_rec_model

pytestmark = pytest.mark.gpu

PREC, FREC, SREC = PACKET_REC_DTYPE.itemsize, FEC_REC_DTYPE.itemsize, 16
SREC_DTYPE = np.dtype([("phase", "<u4"), ("score", "<u4"), ("runner_up", "<u4"), ("nfec", "<u4")])
FILL = 0xEE      # every output before the call
SENTINEL = 0xC3  # between and around the streams (test_gpu_packet.PAD bytes of it at both ends)
FEC_FPB = 20     # FEC frames per workgroup


# ---- a stream with what the models say about it ---------------------------------------------------------------------------
class Stream:
    def __init__(self, data, framebytes, fec, phase=0, min_score=0, planted=None):
        self.data = np.asarray(data, np.uint8)
        assert self.data.size % framebytes == 0
        self.framebytes, self.fec, self.phase, self.min_score, self.planted = framebytes, fec, phase, min_score, planted
        self.nframes, self.nslots = self.data.size // framebytes, self.data.size // SLOT
        self._model = None

    def model(self):
        """(scores or None, stream record, bytes after, FEC records, packet records); computed once"""
        if self._model is None:
            scores = sync_model(self.data) if self.fec == FEC_SEARCH else None
            srec = stream_rec_model(self.fec, self.phase, self.min_score, self.nslots, scores)
            if srec[0] == NO_PHASE:
                after, frec = self.data, np.zeros(0, FEC_REC_DTYPE)
            else:
                after, frec = fec_stream_model(self.data, srec[0])
            assert len(frec) == srec[3]
            self._model = (scores, srec, after, frec, packets_model(after, self.framebytes))
        return self._model


def plant_headers(st, phase, frames):
    """the nine FEC packet headers that `frames` FEC frames from slot `phase` on would carry, and those of the frame in front
    of them, written over whatever the slots hold (inside the stream only)"""
    for f in range(-1, frames):
        for c in range(9):
            i = phase + FEC_SLOTS * f + 94 + c
            if 0 <= i < st.size // SLOT:
                st[SLOT * i:SLOT * i + 2] = fec_hdr(c)
    return st


def damage(rng, st, phase, frames, max_err):
    """the given FEC frames of the stream replaced by random_damaged_frame's: rows with 0 ... max_err byte errors"""
    for f in frames:
        o = SLOT * (phase + FEC_SLOTS * f)
        st[o:o + FEC_FRAME_BYTES] = random_damaged_frame(rng, max_err)
    return st


# ---- running ------------------------------------------------------------------------------------------------------------
def table_of(V, streams, residues=None, order=None):
    """the streams laid out in address order with sentinel bytes between them, stream k at an offset that is residues[k] mod
    16 -> (the table in `order`, host image of the guarded allocation)"""
    parts, offsets, cur = [], [], 0
    for k, s in enumerate(streams):
        gap = 8 + (0 if residues is None else (residues[k] - (cur + 8)) % 16)
        parts.append(np.full(gap, SENTINEL, np.uint8))
        offsets.append(cur + gap)
        parts.append(s.data)
        cur += gap + s.data.size
    parts.append(np.full(8, SENTINEL, np.uint8))
    if residues is not None:
        assert [o % 16 for o in offsets] == [r % 16 for r in residues]
    order = list(range(len(streams))) if order is None else list(order)
    tab = np.zeros(len(streams), V.PKT_STREAM_DTYPE)
    for j, k in enumerate(order):
        s = streams[k]
        tab[j] = (offsets[k], s.framebytes, s.nframes, s.fec, s.phase, s.min_score, 0)
    return tab, np.concatenate(parts), [streams[k] for k in order], [offsets[k] for k in order]


def filled(torch, nbytes):
    """nbytes of output between two 16-byte guards, all FILL -> tensor"""
    return torch.full((nbytes + 32,), FILL, dtype=torch.uint8, device="cuda")


def run_table(V, torch, tab, image, with_score=True, base_offset=0):
    """-> (bytes of the whole guarded allocation, d_srec, d_fec, d_rec, d_score as host arrays, guards included)"""
    lay = V.packet_table_layout(tab)
    n = len(tab)
    d, host = guarded(image, base_offset)
    assert int(lay["bytes_end"]) <= image.size
    d_srec = filled(torch, n * SREC)
    d_fec = filled(torch, int(lay["nfecrec"]) * FREC)
    d_rec = filled(torch, int(lay["nrec"]) * PREC)
    d_score = filled(torch, n * FEC_SLOTS * 4)
    V.packet_table_dev(d[PAD:], tab, d_srec[16:], d_fec[16:] if int(lay["nfecrec"]) else None, d_rec[16:],
                       d_score[16:] if with_score else None)
    torch.cuda.synchronize()
    return d.cpu().numpy(), host, d_srec.cpu().numpy(), d_fec.cpu().numpy(), d_rec.cpu().numpy(), d_score.cpu().numpy()


def expected(tab, image, streams, offsets):
    """what run_table must return, by the models"""
    rec_index, fec_index, nrec, nfecrec, _ = layout_model([tuple(int(v) for v in row) for row in tab.tolist()])
    n = len(streams)
    host = np.concatenate([np.full(PAD, SENTINEL, np.uint8), image, np.full(PAD, SENTINEL, np.uint8)])
    srec = np.full(n * SREC + 32, FILL, np.uint8)
    fec = np.full(nfecrec * FREC + 32, FILL, np.uint8)
    rec = np.full(nrec * PREC + 32, FILL, np.uint8)
    score = np.full(n * FEC_SLOTS * 4 + 32, FILL, np.uint8)
    score[16:-16] = 0
    for k, s in enumerate(streams):
        sc, sr, after, frec, prec = s.model()
        host[PAD + offsets[k]:PAD + offsets[k] + after.size] = after
        srec[16 + SREC * k:16 + SREC * (k + 1)] = np.array([sr], SREC_DTYPE).view(np.uint8)
        o = 16 + FREC * fec_index[k]
        fec[o:o + FREC * len(frec)] = frec.view(np.uint8).reshape(-1)
        o = 16 + PREC * rec_index[k]
        rec[o:o + PREC * s.nslots] = prec.view(np.uint8).reshape(-1)
        if sc is not None:
            score[16 + 4 * FEC_SLOTS * k:16 + 4 * FEC_SLOTS * (k + 1)] = sc.astype("<u4").view(np.uint8)
    return host, srec, fec, rec, score


def first_diff(a, b):
    return np.flatnonzero(a != b)[:8].tolist()


def check_table(V, torch, streams, residues=None, order=None, with_score=True, base_offset=0):
    tab, image, streams, offsets = table_of(V, streams, residues, order)
    got_bytes, host, srec, fec, rec, score = run_table(V, torch, tab, image, with_score, base_offset)
    w_bytes, w_srec, w_fec, w_rec, w_score = expected(tab, image, streams, offsets)
    assert host.size == w_bytes.size
    assert np.array_equal(srec, w_srec), ("stream records", srec[16:-16].view(SREC_DTYPE), w_srec[16:-16].view(SREC_DTYPE))
    if with_score:
        assert np.array_equal(score, w_score), ("scores", first_diff(score, w_score))
    else:
        assert (score == FILL).all()
    assert np.array_equal(fec, w_fec), ("FEC records, guards and records past nfec", first_diff(fec, w_fec))
    assert np.array_equal(got_bytes, w_bytes), ("stream bytes and the sentinels around them", first_diff(got_bytes, w_bytes))
    assert np.array_equal(rec, w_rec), ("packet records", first_diff(rec, w_rec))
    return {"bytes": got_bytes, "srec": srec, "fec": fec, "rec": rec, "score": score, "tab": tab, "streams": streams, "offsets": offsets}


def per_stream_calls(V, torch, s, offset=0):
    """the recipe the table call replaces, on a copy of the stream -> (stream record, bytes after, FEC records, packet records)"""
    d, _ = guarded(s.data, offset)
    ds = d[PAD:PAD + s.data.size]
    phase, score, runner_up = NO_PHASE, 0, 0
    if s.fec == FEC_SEARCH:
        d_score = torch.zeros(FEC_SLOTS, dtype=torch.int32, device="cuda")
        V.packet_fec_sync_dev(ds, s.nslots, d_score)
        phase, score, runner_up = pick_model(d_score.cpu().numpy().astype(np.uint32), s.min_score)
    elif s.fec == FEC_PHASE:
        phase = s.phase
    nfec = 0 if phase == NO_PHASE else V.packet_fec_count(s.nslots, phase)
    d_fec = torch.zeros(max(nfec, 1) * FREC, dtype=torch.uint8, device="cuda")
    if phase != NO_PHASE:
        V.packet_fec_dev(ds, ds, s.nslots, phase, d_fec)
    d_rec = torch.zeros(s.nslots * PREC, dtype=torch.uint8, device="cuda")
    V.packets_dev(ds, s.framebytes, s.nframes, d_rec)
    torch.cuda.synchronize()
    return (phase, score, runner_up, nfec), ds.cpu().numpy(), d_fec.cpu().numpy()[:nfec * FREC], d_rec.cpu().numpy()


def check_against_per_stream_calls(V, torch, got):
    """the outputs of check_table against the three per-stream calls, stream by stream"""
    tab, ordered, offsets = got["tab"], got["streams"], got["offsets"]
    got_bytes, srec, fec, rec = got["bytes"], got["srec"], got["fec"], got["rec"]
    rec_index, fec_index, _, _, _ = layout_model([tuple(int(v) for v in row) for row in tab.tolist()])
    for k, s in enumerate(ordered):
        sr, after, frec, prec = per_stream_calls(V, torch, s, offset=k % 4)
        assert srec[16 + SREC * k:16 + SREC * (k + 1)].view(SREC_DTYPE)[0].tolist() == tuple(sr), k
        assert np.array_equal(got_bytes[PAD + offsets[k]:PAD + offsets[k] + after.size], after), k
        assert np.array_equal(fec[16 + FREC * fec_index[k]:16 + FREC * fec_index[k] + frec.size], frec), k
        assert np.array_equal(rec[16 + PREC * rec_index[k]:16 + PREC * (rec_index[k] + s.nslots)], prec), k


# ---- the streams of the FEC count cases, built and modelled once --------------------------------------------------------------
@pytest.fixture(scope="module")
def fec_streams():
    """nfec 0, 1, 19, 20, 21 and 41 at the found phases 60, 0, 1, 93, 94 and 102; every stream ends in a partial frame.
    (slots per logical frame, slots, planted phase, nfec, the host's bound nslots // 103)"""
    rng = np.random.default_rng(2501)
    shapes = [(8, 152, 60, 0, 1), (4, 108, 0, 1, 1), (8, 1960, 1, 19, 19), (3, 2166, 93, 20, 21), (48, 2304, 94, 21, 22),
              (8, 4328, 102, 41, 42)]
    out = []
    for S, nslots, phase, nfec, bound in shapes:
        st = plant_headers(build_framed_stream(rng, nfec, phase, nslots, S), phase, nfec)
        if nfec == 19:
            damage(rng, st, phase, [0, 7, 18], 3)        # correctable rows only
        if nfec == 20:
            damage(rng, st, phase, [5, 19], 12)          # rows beyond correction among them
        if nfec == 41:
            damage(rng, st, phase, range(20, 41), 12)    # a clean workgroup, a damaged one, and a last one of one frame
        s = Stream(st, SLOT * S, FEC_SEARCH, planted=phase)
        assert fec_count(nslots, phase) == nfec and nslots // FEC_SLOTS == bound
        out.append(s)
    return out


def test_fec_counts_around_the_workgroup(V, torch_cuda, fec_streams):
    """phases found on the device are the planted ones; a stream whose found phase gives fewer frames than the host's bound
    writes exactly nfec records (check_table: the reserved records behind them keep their bytes)"""
    for s in fec_streams:
        sc, sr, after, frec, _ = s.model()
        assert sr[0] == s.planted and sr[3] == fec_count(s.nslots, s.planted) and sr[1] > sr[2]
    nerr = np.concatenate([s.model()[3]["nerr"].reshape(-1) for s in fec_streams])
    assert (nerr == -1).any() and (nerr == 0).any() and (nerr > 0).any()
    clean_wg = fec_streams[5].model()[3]["nerr"]
    assert not clean_wg[:FEC_FPB].any() and clean_wg[FEC_FPB:].any() and clean_wg[2 * FEC_FPB:].any()
    got = check_table(V, torch_cuda, fec_streams, residues=[3, 0, 15, 8, 1, 6], order=[2, 5, 0, 3, 1, 4])
    phases = got["srec"][16:-16].view(SREC_DTYPE)["phase"].tolist()
    assert phases == [1, 102, 60, 93, 0, 94]


@pytest.mark.parametrize("which", range(6))
def test_one_stream_table_equals_the_per_stream_calls(V, torch_cuda, fec_streams, which):
    s = fec_streams[which]
    for with_score in (True, False):
        got = check_table(V, torch_cuda, [s], residues=[which + 5], with_score=with_score)
        check_against_per_stream_calls(V, torch_cuda, got)


# ---- stream boundaries inside a workgroup -----------------------------------------------------------------------------------
def test_stream_boundaries_inside_a_workgroup(V, torch_cuda):
    """framebytes 24, 72, 192 and 1152 with 1, 3 and 7 logical frames, and four more, at every offset mod 16: one wavefront
    round is a whole stream for most of them, so the four wavefronts of a packets workgroup fall on different streams and
    streams end in the middle of a workgroup"""
    rng = np.random.default_rng(2502)
    shapes = [(fb, nf) for nf in (1, 3, 7) for fb in (24, 72, 192, 1152)] + [(1152, 3), (24, 7), (72, 65), (192, 9)]
    streams = []
    for k, (fb, nf) in enumerate(shapes):
        S, nslots = fb // SLOT, nf * fb // SLOT
        if nslots >= 112:
            phase = int(rng.integers(0, min(FEC_SLOTS - 1, nslots - FEC_SLOTS) + 1))
            st = plant_headers(build_framed_stream(rng, 1, phase, nslots, S), phase, 1)
            streams.append(Stream(damage(rng, st, phase, [0], 4), fb, FEC_SEARCH, planted=phase))
        else:
            st = build_framed_stream(rng, 0, 0, nslots, S)
            streams.append(Stream(st, fb, (FEC_NONE, FEC_SEARCH)[k % 2]))
    assert sum(1 for s in streams if s.planted is not None) >= 3
    for s in streams:
        if s.planted is not None:
            assert s.model()[1][0] == s.planted and s.model()[1][3] >= 1
    # packet passes of one wavefront each: 64 // S frames a pass
    passes = [-(-s.nframes // (64 // (s.framebytes // SLOT))) for s in streams]
    assert passes.count(1) >= 8 and max(passes) >= 3 and sum(passes) % 4 != 0
    check_table(V, torch_cuda, streams, residues=list(range(16)))
    check_table(V, torch_cuda, streams, residues=list(range(15, -1, -1)), order=rng.permutation(16), with_score=False, base_offset=1)


# ---- all three modes in one table ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed_streams():
    rng = np.random.default_rng(2503)
    out = []
    for fec, phase, S in ((FEC_NONE, 7, 8), (FEC_PHASE, 100, 2), (FEC_SEARCH, 40, 8), (FEC_PHASE, 0, 48)):
        nslots = -(-(phase + 2 * FEC_SLOTS + 11) // S) * S
        st = damage(rng, plant_headers(build_framed_stream(rng, 2, phase, nslots, S), phase, 2), phase, [1], 6)
        out.append(Stream(st, SLOT * S, fec, phase if fec == FEC_PHASE else 0, planted=phase))
    return out


def test_all_three_modes_in_one_table(V, torch_cuda, mixed_streams):
    none = mixed_streams[0]
    _, sr, after, frec, prec = none.model()
    assert sr == (NO_PHASE, 0, 0, 0) and after is none.data and len(frec) == 0
    assert fec_stream_model(none.data, none.planted)[1]["nerr"].any(), "the FEC_NONE stream does hold damaged rows"
    assert int((prec["kind"] == PKT_FEC).sum()) >= 9, "its FEC packets appear as VIT_PKT_FEC records"
    assert mixed_streams[2].model()[1][0] == 40
    got = check_table(V, torch_cuda, mixed_streams, residues=[5, 9, 2, 12])
    check_against_per_stream_calls(V, torch_cuda, got)
    check_table(V, torch_cuda, mixed_streams, order=[3, 2, 1, 0], with_score=False)


def test_two_runs_give_the_same_bytes(V, torch_cuda, mixed_streams):
    tab, image, _, _ = table_of(V, mixed_streams, [1, 2, 3, 4])
    a = run_table(V, torch_cuda, tab, image)
    b = run_table(V, torch_cuda, tab, image)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- the pick ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_score", [True, False])
def test_phase_pick(V, torch_cuda, with_score):
    """two equal maxima: the smallest phase wins and runner_up equals score; no header at all and a score below min_score:
    no phase, the stream untouched (its damaged rows stay) and still walked for packets"""
    rng = np.random.default_rng(2504)
    streams = []
    for p1, p2 in ((5, 70), (66, 90), (0, 64)):  # both maxima among phases 0 ... 63, both above, one on either side
        nslots = p2 + 2 * FEC_SLOTS + 8
        st = plant_headers(damage(rng, build_framed_stream(rng, 2, p1, nslots, 1), p1, [0], 5), p1, 2)
        mine = sync_model(st)[p1]
        other = 0
        for f in range(-1, 3):  # headers that only phase p2 counts, until it has as many
            for c in range(9):
                i = p2 + FEC_SLOTS * f + 94 + c
                if 0 <= i < nslots and other < mine and tuple(st[SLOT * i:SLOT * i + 2]) != fec_hdr(c):
                    st[SLOT * i:SLOT * i + 2] = fec_hdr(c)
                    other += 1
        s = Stream(st, SLOT, FEC_SEARCH, planted=p1)
        sc = s.model()[0]
        assert sc[p1] == sc[p2] == sc.max() and s.model()[1][:3] == (p1, int(sc[p1]), int(sc[p1]))
        streams.append(s)
    plain = Stream(build_framed_stream(rng, 0, 0, 240, 8), 192, FEC_SEARCH)
    assert plain.model()[1] == (NO_PHASE, 0, 0, 0)
    streams.append(plain)
    st = damage(rng, plant_headers(build_framed_stream(rng, 1, 9, 120, 8), 9, 1), 9, [0], 6)
    low = Stream(st, 192, FEC_SEARCH, min_score=int(sync_model(st).max()) + 1)
    assert low.model()[1][0] == NO_PHASE and low.model()[1][1] >= 9 and low.model()[2] is low.data
    assert fec_stream_model(st, 9)[1]["nerr"].any()
    streams.append(low)
    streams.append(Stream(st.copy(), 192, FEC_SEARCH, min_score=int(sync_model(st).max()), planted=9))  # exactly min_score
    assert streams[-1].model()[1][0] == 9
    check_table(V, torch_cuda, streams, residues=[7, 7, 0, 11, 4, 13], with_score=with_score)


# ---- table shape ------------------------------------------------------------------------------------------------------------
def test_64_streams_of_one_frame(V, torch_cuda):
    """no stream can hold an FEC frame: nfecrec is 0 and d_fec NULL"""
    rng = np.random.default_rng(2505)
    streams = []
    for k in range(64):
        S = (1, 2, 3, 8, 47, 48)[k % 6]
        st = build_framed_stream(rng, 0, 0, S, S)
        if k % 5 == 0:
            st[SLOT * (S - 1):SLOT * (S - 1) + 2] = fec_hdr(0)  # the last slot carries an FEC header: phase S + 8 scores 1
        streams.append(Stream(st, SLOT * S, (FEC_SEARCH, FEC_NONE, FEC_PHASE)[k % 3], phase=(k % FEC_SLOTS) if k % 3 == 2 else 0))
    tab = table_of(V, streams)[0]
    assert int(V.packet_table_layout(tab)["nfecrec"]) == 0
    assert any(s.model()[1][0] not in (NO_PHASE, 0) and s.fec == FEC_SEARCH for s in streams)
    check_table(V, torch_cuda, streams, residues=[(5 * k) % 16 for k in range(64)], order=rng.permutation(64))


# ---- arguments ------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(V, torch_cuda, mixed_streams):
    torch = torch_cuda
    L = V.lib()
    tab, image, _, _ = table_of(V, mixed_streams)
    lay = V.packet_table_layout(tab)
    assert int(lay["nfecrec"]) > 0
    d, host = guarded(image, 0)
    outs = [filled(torch, len(tab) * SREC), filled(torch, int(lay["nfecrec"]) * FREC), filled(torch, int(lay["nrec"]) * PREC),
            filled(torch, len(tab) * FEC_SLOTS * 4)]
    p_bytes = d[PAD:].data_ptr()
    srec, fec, rec, score = (o[16:].data_ptr() for o in outs)
    bad = tab.copy()
    bad["offset"][1] = bad["offset"][0] + 24
    calls = [(p_bytes, tab, srec, fec, rec + 2, score), (p_bytes, tab, srec + 1, fec, rec, score), (p_bytes, tab, srec, fec + 2, rec, score),
             (p_bytes, tab, srec, fec, rec, score + 3), (p_bytes, tab, srec, None, rec, score), (None, tab, srec, fec, rec, score),
             (p_bytes, tab, None, fec, rec, score), (p_bytes, tab, srec, fec, None, score), (p_bytes, bad, srec, fec, rec, score),
             (p_bytes, tab[:0], srec, fec, rec, score)]
    for b, t, s, f, r, sc in calls:
        rc = L.vit_packet_table_dev(b, t.ctypes.data if len(t) else None, len(t), s, f, r, sc, None)
        assert rc == 1 and "vit_packet_table_dev" in V.last_error(), V.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), host)
    assert all(bool((o == FILL).all()) for o in outs)
    with pytest.raises(V.ViterbiError):
        V.packet_table_dev(d[PAD:], bad, outs[0][16:], outs[1][16:], outs[2][16:])
