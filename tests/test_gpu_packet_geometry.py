"""GPU: the launch geometry of packet mode - vit_packets_dev at every frame size S = 1 ... 48 slots (64 // S frames per
wavefront, the dead-lane tail, the chain walk) and at every byte offset in 16 (the image phase, the v_alignbyte shift),
with the record edge cases in every stream; vit_packet_fec_sync_dev with more than one workgroup.  Whole record arrays
against packets_model, scores against the sync model, byte for byte."""
import numpy as np
import pytest
import torch  # noqa: F401  (torch's runtime first, as when the whole suite is collected)

import fecdirect as fd
from test_gpu_packet import run_packets, run_sync
from test_packet_host import (ADDR_PADDING, FEC_SLOTS, PKT_CONT, PKT_DATA, PKT_FEC, PKT_OVERRUN, PKT_PADDING, SLOT, crc16, fec_hdr,
                              make_packet, packets_model, random_packets, same)

gpu = pytest.mark.gpu  # (the builders' own test below needs no device)

WAVE = 64
KINDS = {PKT_CONT, PKT_DATA, PKT_PADDING, PKT_FEC, PKT_OVERRUN}
NVARIANTS = 6


def random_mix(rng, total, first=None):
    """packet lengths 1 ... 4 that fill `total` slots, the first one `first` where that fits"""
    mix = []
    while sum(mix) < total:
        room = min(4, total - sum(mix))
        mix.append(min(first, room) if first and not mix else int(rng.integers(1, room + 1)))
    return mix


def packets_of(rng, mix):
    return random_packets(rng, mix) if mix else np.zeros(0, np.uint8)


def fec_slot(rng, lenbits, valid_crc):
    s = rng.integers(0, 256, SLOT, dtype=np.uint8)
    s[0], s[1] = fec_hdr(int(rng.integers(0, 16)))
    s[0] |= lenbits << 6
    if valid_crc:  # as a data packet of one slot its CRC would hold
        c = crc16(s[:SLOT - 2])
        s[SLOT - 2], s[SLOT - 1] = c >> 8, c & 255
    return s


def variant_frame(rng, S, v):
    """one logical frame of S slots: 0 plain (a packet of two slots in front where they fit), 1 a flipped bit behind the
    header of every packet, 2 the last packet lengthened past the frame's end, 3 an address-1022 slot with length bits
    1 ... 3 in mid-frame, 4 a padding packet with a bad CRC, 5 an address-1022 slot whose 22 bytes carry their CRC"""
    if v in (3, 5):
        q = int(rng.integers(1, S - 1)) if S >= 3 else 0
        slot = fec_slot(rng, int(rng.integers(1, 4)) if v == 3 else int(rng.integers(0, 4)), v == 5)
        return np.concatenate([packets_of(rng, random_mix(rng, q)), slot, packets_of(rng, random_mix(rng, S - q - 1))])
    if v == 2:
        fr = packets_of(rng, random_mix(rng, S - 1) + [1])
        fr[SLOT * (S - 1)] |= int(rng.integers(1, 4)) << 6
        return fr
    mix = random_mix(rng, S, first=2)
    fr = packets_of(rng, mix)
    starts = np.cumsum([0] + mix[:-1])
    if v == 1:
        for a, n in zip(starts, mix):
            fr[SLOT * int(a) + int(rng.integers(3, SLOT * n))] ^= 1 << int(rng.integers(0, 8))
    if v == 4:
        k = int(rng.integers(0, len(mix)))
        a, n = int(starts[k]), mix[k]
        fr[SLOT * a:SLOT * (a + n)] = make_packet(rng, n, ADDR_PADDING)
        fr[SLOT * a + int(rng.integers(3, SLOT * n))] ^= 1 << int(rng.integers(0, 8))
    return fr


def stream_of(rng, S, nframes):
    return np.concatenate([variant_frame(rng, S, k % NVARIANTS) for k in range(nframes)])


def image_phases(S, nframes, offset):
    """the 16-byte phases a = (address of a wavefront's first frame) mod 16 that a launch meets"""
    G = WAVE // S
    return {(offset + fw * S * SLOT) % 16 for fw in range(0, nframes, G)}


def test_packet_variants_are_what_they_say():
    """(no device) the model on the edge cases the streams carry"""
    rng = np.random.default_rng(1)
    for S in (1, 2, 3, 7, 48):
        r = packets_model(variant_frame(rng, S, 1), SLOT * S)
        assert not r["crc_ok"].any() and (r["kind"] != PKT_OVERRUN).all()
        r = packets_model(variant_frame(rng, S, 2), SLOT * S)
        assert r["kind"][-1] == PKT_OVERRUN and (r["kind"][:-1] != PKT_OVERRUN).all()
        for v in (3, 5):
            fr = variant_frame(rng, S, v)
            r = packets_model(fr, SLOT * S)
            k = np.flatnonzero(r["kind"] == PKT_FEC)
            assert k.size == 1 and r["crc_ok"][k[0]] == 0 and r["nslots"][k[0]] == 1 and (S < 3 or 0 < k[0] < S - 1)
            assert (fr[SLOT * k[0]] >> 6 != 0) if v == 3 else \
                crc16(fr[SLOT * k[0]:SLOT * k[0] + 22]) == (int(fr[SLOT * k[0] + 22]) << 8 | int(fr[SLOT * k[0] + 23]))
            assert (r["kind"] != PKT_OVERRUN).all()
        r = packets_model(variant_frame(rng, S, 4), SLOT * S)
        k = np.flatnonzero(r["kind"] == PKT_PADDING)
        assert k.size == 1 and r["crc_ok"][k[0]] == 0 and int(r["crc_ok"].sum()) == int((r["kind"] == PKT_DATA).sum())


@gpu
def test_packets_every_frame_size(V, torch_cuda):
    phases, shifts = set(), set()
    for S in range(1, 49):
        rng = np.random.default_rng(4800 + S)
        G = WAVE // S
        nframes = 9 * G + 2  # two full workgroups, a full wavefront, one of two frames (G > 2), idle ones
        st = stream_of(rng, S, nframes)
        want = packets_model(st, SLOT * S)
        if S >= 3:
            assert set(want["kind"].tolist()) == KINDS, S
        fec = want["kind"] == PKT_FEC
        assert fec.any() and not want["crc_ok"][fec].any()
        assert (want["crc_ok"][want["kind"] == PKT_PADDING] == 0).any()
        for offset in ((5 * S) % 16, 2):
            phases |= image_phases(S, nframes, offset)
            shifts |= {a & 3 for a in image_phases(S, nframes, offset)}
            got = run_packets(V, torch_cuda, st, SLOT * S, offset)
            assert same(got, want), (S, offset, np.flatnonzero(got != want)[:8])
    assert {(5 * S) % 16 for S in range(1, 49)} == set(range(16)) == phases
    assert 2 in shifts and shifts == {0, 1, 2, 3}


@gpu
@pytest.mark.parametrize("S", [1, 3, 5, 16, 21, 48])
def test_packets_every_offset(V, torch_cuda, S):
    rng = np.random.default_rng(1600 + S)
    nframes = 4 * (WAVE // S) + 1
    st = stream_of(rng, S, nframes)
    want = packets_model(st, SLOT * S)
    for offset in range(16):
        got = run_packets(V, torch_cuda, st, SLOT * S, offset)
        assert same(got, want), (S, offset, np.flatnonzero(got != want)[:8])


@gpu
@pytest.mark.parametrize("nslots", [1024, 1025, 4096, 4097, 20000])
def test_sync_scores_across_workgroups(V, torch_cuda, nslots):
    rng = np.random.default_rng(nslots)
    for phase, offset in ((0, 0), (50, 1), (102, 2)):
        st = fd.sync_stream(rng, nslots, phase, stray=40)
        want = fd.sync_model_fast(st)
        assert int(want.sum()) >= 9 * (nslots // FEC_SLOTS - 1)
        if nslots == 20000:
            assert int(np.argmax(want)) == phase
        got = run_sync(V, torch_cuda, st, offset)
        assert np.array_equal(got, want), (phase, np.flatnonzero(got != want)[:8])
        if nslots == 20000:
            assert int(np.argmax(got)) == phase
    st = rng.integers(0, 256, SLOT * nslots, dtype=np.uint8)
    assert np.array_equal(run_sync(V, torch_cuda, st, 3), fd.sync_model_fast(st))
