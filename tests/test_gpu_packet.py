"""GPU: packet mode (vit_packets_dev, vit_packet_fec_dev, vit_packet_fec_sync_dev) against the model and the builders of
tests/test_packet_host.py, byte for byte: sentinel bytes around every output, inputs unchanged, base offsets 0, 1 and 3."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (torch's runtime first, as when the whole suite is collected)

from test_gpu_dab import dev
from test_packet_host import (ADDR_PADDING, COLS, FEC_DATA_BYTES, FEC_FRAME_BYTES, FEC_REC_DTYPE, FEC_SLOTS, IDX, NCODE, NPAR,
                              PACKET_REC_DTYPE, PKT_CONT, PKT_DATA, PKT_FEC, PKT_OVERRUN, PKT_PADDING, ROWS, SLOT,
                              build_fec_frame, build_framed_stream, encode_rows, fec_frame_model, fec_hdr, frame_of_rows,
                              length_mixes, make_packet, miscorrection_row, packets_model, padding_root_row, plant,
                              random_packets, same, sync_model)

pytestmark = pytest.mark.gpu

PREC, FREC = PACKET_REC_DTYPE.itemsize, FEC_REC_DTYPE.itemsize  # 8, 16
FEC_FPB = 20  # FEC frames per workgroup of vit_fec_kernel
PAD = 32


# ---- running ----------------------------------------------------------------------------------------------------------
def guarded(host_bytes, offset):
    """the bytes between two runs of PAD sentinel bytes, `offset` bytes into an allocation -> (whole view, host image)"""
    host = np.concatenate([np.full(PAD, 0xC3, np.uint8), np.asarray(host_bytes, np.uint8), np.full(PAD, 0xC3, np.uint8)])
    return dev(host, offset), host


def run_packets(V, torch, stream, framebytes, offset=0):
    stream = np.asarray(stream, np.uint8)
    nframes = stream.size // framebytes
    n = nframes * (framebytes // SLOT)
    d, host = guarded(stream, offset)
    d_rec = torch.full(((n + 2) * PREC,), 0xEE, dtype=torch.uint8, device="cuda")
    V.packets_dev(d[PAD:], framebytes, nframes, d_rec[PREC:])
    torch.cuda.synchronize()
    rec = d_rec.cpu().numpy()
    assert (rec[:PREC] == 0xEE).all() and (rec[(n + 1) * PREC:] == 0xEE).all()
    assert np.array_equal(d.cpu().numpy(), host)
    return rec[PREC:(n + 1) * PREC].view(PACKET_REC_DTYPE)


def run_fec(V, torch, stream, phase, off_in=0, off_out=0):
    """in place and out of place: the same bytes and records -> (stream after, records)"""
    stream = np.asarray(stream, np.uint8)
    n, nslots = stream.size, stream.size // SLOT
    nfec = V.packet_fec_count(nslots, phase)
    results = []
    for inplace in (True, False):
        d, host = guarded(stream, off_in)
        d_fec = torch.full(((nfec + 2) * FREC,), 0xEE, dtype=torch.uint8, device="cuda")
        if inplace:
            d_o, ohost = d, host
        else:
            d_o, ohost = guarded(np.full(n, 0x5A, np.uint8), off_out)
        V.packet_fec_dev(d[PAD:PAD + n], d_o[PAD:PAD + n], nslots, phase, d_fec[FREC:])
        torch.cuda.synchronize()
        out, rec = d_o.cpu().numpy(), d_fec.cpu().numpy()
        assert np.array_equal(out[:PAD], ohost[:PAD]) and np.array_equal(out[PAD + n:], ohost[PAD + n:])
        assert (rec[:FREC] == 0xEE).all() and (rec[(nfec + 1) * FREC:] == 0xEE).all()
        if not inplace:
            assert np.array_equal(d.cpu().numpy(), host)
        results.append((out[PAD:PAD + n].copy(), rec[FREC:(nfec + 1) * FREC].view(FEC_REC_DTYPE).copy()))
    assert np.array_equal(results[0][0], results[1][0]) and same(results[0][1], results[1][1])
    return results[0]


def run_sync(V, torch, stream, offset=0):
    stream = np.asarray(stream, np.uint8)
    d, host = guarded(stream, offset)
    d_score = torch.full((FEC_SLOTS + 2,), 0x7EEEEEEE, dtype=torch.int32, device="cuda")
    V.packet_fec_sync_dev(d[PAD:], stream.size // SLOT, d_score[1:])
    torch.cuda.synchronize()
    sc = d_score.cpu().numpy()
    assert sc[0] == 0x7EEEEEEE and sc[-1] == 0x7EEEEEEE and np.array_equal(d.cpu().numpy(), host)
    return sc[1:-1].astype(np.uint32)


# ---- packets ------------------------------------------------------------------------------------------------------------
def with_flips(frame, mix):
    """the frame and, per packet, copies with one bit flipped in the first header byte's low bits, the last data byte and
    each CRC byte -> (copies, per copy the index of the packet whose CRC must fail, -1 for none)"""
    out, hit = [frame], [-1]
    starts = np.cumsum([0] + list(mix))
    for k, n in enumerate(mix):
        a, e = SLOT * int(starts[k]), SLOT * int(starts[k] + n)
        for pos, bit in ((a, 0x10), (e - 3, 0x01), (e - 2, 0x10), (e - 1, 0x04)):
            c = frame.copy()
            c[pos] ^= bit
            out.append(c)
            hit.append(k)
    return out, hit


def mixes_for(slots):
    if slots <= 5:
        return length_mixes(slots)
    return [[1] * 48, [4] * 12, [1, 2, 3, 4] * 4 + [4, 4], [3] * 16, [2, 4] * 8]


@pytest.mark.parametrize("framebytes", [24, 48, 72, 96, 120, 1152])
def test_packets_every_mix_and_flip(V, torch_cuda, framebytes):
    rng = np.random.default_rng(framebytes)
    S = framebytes // SLOT
    frames, want_ok = [], []
    for mix in mixes_for(S):
        copies, hit = with_flips(random_packets(rng, mix), mix)
        frames += copies
        want_ok += [[0 if k == h else 1 for k in range(len(mix))] for h in hit]
    for nframes, offset in ((1, 0), (2, 1), (67, 3), (len(frames), 1)):
        st = np.concatenate([frames[k % len(frames)] for k in range(nframes)])
        want = packets_model(st, framebytes)
        if nframes == len(frames):
            starts = want["kind"] == PKT_DATA
            assert want["crc_ok"][starts].tolist() == [x for row in want_ok for x in row]
            assert not (want["kind"] == PKT_OVERRUN).any()
        got = run_packets(V, torch_cuda, st, framebytes, offset)
        assert same(got, want), (nframes, offset, np.flatnonzero(got != want)[:8])


@pytest.mark.parametrize("framebytes", [96, 120, 1152])
def test_packets_flipped_lengths_and_kinds(V, torch_cuda, framebytes):
    """the length field of the first and of the last packet of a frame rewritten to every other value (shorter, longer,
    past the frame's end); padding and FEC packets between data packets"""
    rng = np.random.default_rng(100 + framebytes)
    S = framebytes // SLOT
    frames = []
    for mix in mixes_for(S)[:6]:
        base = random_packets(rng, mix)
        last = SLOT * (S - mix[-1])
        for pos in (0, last):
            for ln in range(4):
                c = base.copy()
                c[pos] = (c[pos] & 0x3F) | ln << 6
                frames.append(c)
    fr = random_packets(rng, mixes_for(S)[0])
    fr[:SLOT * mixes_for(S)[0][0]] = make_packet(rng, mixes_for(S)[0][0], ADDR_PADDING)
    fr[framebytes - SLOT:framebytes - SLOT + 2] = fec_hdr(7)
    bad = fr.copy()
    bad[framebytes - SLOT] |= 0xC0  # address 1022 with length bits set: still one slot
    frames += [fr, bad]
    st = np.concatenate(frames)
    want = packets_model(st, framebytes)
    assert set(want["kind"].tolist()) == {PKT_CONT, PKT_DATA, PKT_PADDING, PKT_FEC, PKT_OVERRUN}
    for offset in (0, 3):
        got = run_packets(V, torch_cuda, st, framebytes, offset)
        assert same(got, want), (offset, np.flatnonzero(got != want)[:8])


# ---- FEC ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool():
    """FEC frames with their model results, computed once: (frames, decoded, records, outcomes seen)"""
    rng = np.random.default_rng(77)
    frames = []

    def rows_with(counts):
        rows = []
        for n in counts:
            cw = encode_rows(rng.integers(0, 256, COLS, dtype=np.uint8))
            rows.append((plant(rng, cw, [int(x) for x in rng.permutation(NCODE)[:n]]), cw))
        return rows

    kinds = []
    for rep in range(3):  # every degree beside every other, 9 and 12 errors among them
        rows = rows_with([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 0])
        order = rng.permutation(ROWS)
        frames.append(frame_of_rows(rng, [rows[k][0] for k in order]))
        kinds.append([rows[k][1] for k in order])
    mis = [miscorrection_row(rng) for _ in range(6)]
    frames.append(frame_of_rows(rng, [m[0] for m in mis] + [padding_root_row(rng) for _ in range(6)]))
    kinds.append([m[1] for m in mis] + [None] * 6)  # (for a miscorrection: the word it must become, not the one sent)
    # errors only in parity; two rows hit in the same column
    cws = encode_rows(rng.integers(0, 256, (ROWS, COLS), dtype=np.uint8))
    par = cws.copy()
    for r in range(ROWS):
        par[r] = plant(rng, par[r], [int(x) for x in COLS + rng.permutation(NPAR)[:r % 9]])
    frames.append(frame_of_rows(rng, list(par)))
    kinds.append(list(cws))
    col = cws.copy()
    for c in (0, 17, 187):
        for r in (2, 3, 11):
            col[r, c] ^= int(rng.integers(1, 256))
    frames.append(frame_of_rows(rng, list(col)))
    kinds.append(list(cws))
    # errors in FEC headers and padding: outside the code
    hp = frame_of_rows(rng, list(plant(rng, cws[r], [3 * r, 100 + r]) for r in range(ROWS)))
    hp[FEC_DATA_BYTES + SLOT * 2] ^= 0x40
    hp[FEC_DATA_BYTES + SLOT * 5 + 1] ^= 0x01
    hp[-6:] = rng.integers(1, 256, 6, dtype=np.uint8)
    frames.append(hp)
    kinds.append(list(cws))
    frames.append(build_fec_frame(rng.integers(0, 256, FEC_DATA_BYTES, dtype=np.uint8)))  # all clean
    kinds.append([None] * ROWS)
    decoded, recs = zip(*(fec_frame_model(f) for f in frames))
    recs = np.concatenate([np.asarray(r).reshape(1) for r in recs])
    assert recs["hdr_ok"][6] == 0x1FF ^ 4 ^ 32 and np.array_equal(decoded[6][-6:], hp[-6:]) and recs["status"][6] == 0
    # the outcomes the inputs hold, by the model
    seen = set(recs["nerr"][:3].reshape(-1).tolist())
    assert seen == set(range(-1, 9)), "clean, nerr 1 ... 8 and no codeword in reach"
    assert recs["nerr"][3].tolist() == [8] * 6 + [-1] * 6, "miscorrected and failed by a padding root"
    for m, r in zip(mis, range(6)):
        sent_plus_w = m[1]
        assert np.array_equal(decoded[3][IDX[r]], sent_plus_w) and not np.array_equal(decoded[3][IDX[r]], m[0])
    for f in (4, 5, 6):
        assert all(np.array_equal(decoded[f][IDX[r]], kinds[f][r]) for r in range(ROWS))
    return list(frames), list(decoded), recs


def fec_case(pool, rng, nfec, phase, tail, first=0):
    """a stream of `phase` slots, nfec frames of the pool and `tail` slots -> (stream, stream after, records)"""
    frames, decoded, recs = pool
    pick = [(first + k) % len(frames) for k in range(nfec)]
    head = rng.integers(0, 256, SLOT * phase, dtype=np.uint8)
    rest = rng.integers(0, 256, SLOT * tail, dtype=np.uint8)
    st = np.concatenate([head] + [frames[k] for k in pick] + [rest])
    want = np.concatenate([head] + [decoded[k] for k in pick] + [rest])
    return st, want, recs[pick] if nfec else np.zeros(0, FEC_REC_DTYPE)


@pytest.mark.parametrize("nfec,phase,tail,off_in,off_out", [
    (1, 0, 0, 0, 0), (2, 1, 1, 1, 1), (FEC_FPB - 1, 102, 102, 3, 3), (FEC_FPB, 0, 1, 0, 16), (FEC_FPB + 1, 1, 0, 1, 3),
    (23, 102, 102, 3, 0), (0, 1, 101, 1, 0), (0, 50, 0, 0, 3)])
def test_fec_against_the_model(V, torch_cuda, pool, nfec, phase, tail, off_in, off_out):
    rng = np.random.default_rng(1000 * nfec + phase)
    if nfec == 0 and tail == 0:
        st, want, wrec = fec_case(pool, rng, 0, 9, 0)  # 9 slots, fewer than the phase
    else:
        st, want, wrec = fec_case(pool, rng, nfec, phase, tail, first=nfec)
    got, rec = run_fec(V, torch_cuda, st, phase, off_in, off_out)
    assert len(rec) == nfec and same(rec, wrec), np.flatnonzero(rec != wrec)[:8]
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


def test_fec_clean_workgroups_beside_damaged(V, torch_cuda, pool):
    """only clean frames in the first workgroup, the damaged ones in the second"""
    frames, decoded, recs = pool
    pick = [len(frames) - 1] * FEC_FPB + list(range(len(frames)))
    st = np.concatenate([frames[k] for k in pick])
    got, rec = run_fec(V, torch_cuda, st, 0, 1, 1)
    assert same(rec, recs[pick]) and np.array_equal(got, np.concatenate([decoded[k] for k in pick]))


# ---- sync -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nslots", [9, 103, 104, 1000])
def test_sync_scores(V, torch_cuda, nslots):
    rng = np.random.default_rng(nslots)
    for phase, offset in ((0, 0), (50, 1), (102, 3)):
        st = rng.integers(0, 256, SLOT * nslots, dtype=np.uint8)
        for i in range(nslots):
            m = (i - phase) % FEC_SLOTS
            if m >= 94:
                st[SLOT * i:SLOT * i + 2] = fec_hdr(m - 94)
        for i in rng.integers(0, nslots, 6):  # headers in the wrong place, and a counter above 8
            st[SLOT * i:SLOT * i + 2] = fec_hdr(int(rng.integers(0, 12)))
        want = sync_model(st)
        if nslots >= 1000:
            assert int(np.argmax(want)) == phase
        got = run_sync(V, torch_cuda, st, offset)
        assert np.array_equal(got, want), (phase, np.flatnonzero(got != want)[:8])
    st = rng.integers(0, 256, SLOT * nslots, dtype=np.uint8)
    assert np.array_equal(run_sync(V, torch_cuda, st, 1), sync_model(st))


# ---- composition ----------------------------------------------------------------------------------------------------------
def test_sync_then_fec_then_packets(V, torch_cuda):
    rng = np.random.default_rng(9)
    phase, S = 3, 8
    st = build_framed_stream(rng, 3, phase, 312, S)
    clean = packets_model(st, SLOT * S)
    assert clean["crc_ok"][clean["kind"] == PKT_DATA].all()
    bad = st.copy()
    for k in range(3):
        o = SLOT * (phase + FEC_SLOTS * k)
        inside = [p for p in range(FEC_DATA_BYTES) if p % SLOT >= 3]  # (length and address stay as they are)
        for pos in rng.permutation(inside)[:10]:
            bad[o + int(pos)] ^= int(rng.integers(1, 256))
    before = run_packets(V, torch_cuda, bad, SLOT * S)
    data = before["kind"] == PKT_DATA
    assert same(before, packets_model(bad, SLOT * S)) and 0 < int((before["crc_ok"][data] == 0).sum()) <= 30
    score = run_sync(V, torch_cuda, bad)
    assert int(np.argmax(score)) == phase and score[phase] == 27
    fixed, rec = run_fec(V, torch_cuda, bad, phase)
    assert (rec["status"] == 0).all() and (rec["hdr_ok"] == 0x1FF).all() and int(rec["nerr"].sum()) == 30
    assert np.array_equal(fixed, st)
    after = run_packets(V, torch_cuda, fixed, SLOT * S)
    assert same(after, clean) and after["crc_ok"][after["kind"] == PKT_DATA].all()
    assert int((after["kind"] == PKT_FEC).sum()) == 27


# ---- arguments ------------------------------------------------------------------------------------------------------------
def test_argument_errors(V, torch_cuda):
    torch = torch_cuda
    L = V.lib()
    d = torch.full((4 * FEC_FRAME_BYTES,), 0x11, dtype=torch.uint8, device="cuda")
    o = torch.full((4 * FEC_FRAME_BYTES,), 0xEE, dtype=torch.uint8, device="cuda")
    ptr, out = C.c_void_p(d.data_ptr()), C.c_void_p(o.data_ptr())
    odd = C.c_void_p(o.data_ptr() + 2)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for fb in (0, 23, 25, 100, 1176, 1153):
        assert L.vit_packets_dev(ptr, fb, 1, out, s) == 1
    assert L.vit_packets_dev(None, 24, 1, out, s) == 1 and L.vit_packets_dev(ptr, 24, 1, None, s) == 1
    assert L.vit_packets_dev(ptr, 24, 1, odd, s) == 1 and L.vit_packets_dev(ptr, 24, -1, out, s) == 1
    assert "vit_packets_dev: bad arguments" in V.last_error()
    assert L.vit_packet_fec_dev(ptr, ptr, 103, 103, out, s) == 1
    assert L.vit_packet_fec_dev(ptr, C.c_void_p(d.data_ptr() + 24), 103, 0, out, s) == 1      # overlapping, unequal
    assert L.vit_packet_fec_dev(ptr, C.c_void_p(d.data_ptr() + 2471), 103, 0, out, s) == 1
    assert L.vit_packet_fec_dev(C.c_void_p(d.data_ptr() + 2471), ptr, 103, 0, out, s) == 1
    assert L.vit_packet_fec_dev(None, ptr, 103, 0, out, s) == 1 and L.vit_packet_fec_dev(ptr, None, 103, 0, out, s) == 1
    assert L.vit_packet_fec_dev(ptr, ptr, 103, 0, None, s) == 1 and L.vit_packet_fec_dev(ptr, ptr, 103, 0, odd, s) == 1
    assert L.vit_packet_fec_dev(ptr, ptr, -1, 0, out, s) == 1
    assert "vit_packet_fec_dev: bad arguments" in V.last_error()
    assert L.vit_packet_fec_sync_dev(None, 9, out, s) == 1 and L.vit_packet_fec_sync_dev(ptr, 9, None, s) == 1
    assert L.vit_packet_fec_sync_dev(ptr, 9, odd, s) == 1 and L.vit_packet_fec_sync_dev(ptr, -1, out, s) == 1
    assert "vit_packet_fec_sync_dev: bad arguments" in V.last_error()
    # empty batches: VIT_OK, nothing written
    assert L.vit_packets_dev(None, 24, 0, None, s) == 0 and L.vit_packet_fec_sync_dev(None, 0, None, s) == 0
    assert L.vit_packet_fec_dev(None, None, 0, 0, None, s) == 0
    torch.cuda.synchronize()
    assert (o.cpu().numpy() == 0xEE).all() and (d.cpu().numpy() == 0x11).all()
