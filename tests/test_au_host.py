"""CPU-only: DAB+ access units (include/viterbi_amd.h, "DAB+ access units") as a numpy / integer model independent of
the library - the superframe header of TS 102 563 clause 5.2, the library's validity rule and the AU CRCs - pinned by
known answers and by crc16_genibus, and the library's host form vit_dabplus_aus_host checked against the model.
tests/test_gpu_au.py uses the same model and builder as its reference."""
import subprocess

import numpy as np
import pytest

from test_dab_host import crc16_genibus, fire_ok_model, with_fire_code

AU_DTYPE = np.dtype([("status", "u1"), ("num_aus", "u1"), ("param", "u1"), ("crc_ok", "u1"), ("au_start", "<u2", (7,)),
                     ("fire_ok", "u1"), ("reserved", "u1")])
AU_OK, AU_RS_FAILED, AU_BAD_HEADER = 0, 1, 2
HEADER_LEN = {2: 5, 3: 6, 4: 8, 6: 11}
# byte 2 per num_aus: (dac_rate, sbr_flag) = (0,1), (1,1), (0,0), (1,0); the other bits are free
PARAM = {2: 0x20, 3: 0x60, 4: 0x00, 6: 0x40}


# ---- the model ------------------------------------------------------------------------------------------------------

def _crc_table():
    t = []
    for b in range(256):
        r = b << 8
        for _ in range(8):
            r = ((r << 1) ^ 0x1021) & 0xFFFF if r & 0x8000 else (r << 1) & 0xFFFF
        t.append(r)
    return t


_CRC_TAB = _crc_table()


def crc16_au(data):
    """CRC-16 0x1021, preset 0xFFFF, MSB first, ones' complement: crc16_genibus by a byte table"""
    r = 0xFFFF
    for b in bytes(data):
        r = ((r << 8) & 0xFFFF) ^ _CRC_TAB[(r >> 8) ^ b]
    return r ^ 0xFFFF


def num_aus_of(param):
    return {(0, 1): 2, (1, 1): 3, (0, 0): 4, (1, 0): 6}[((param >> 6) & 1, (param >> 5) & 1)]


def parse_header(sf):
    """-> (num_aus, au_start[0 .. num_aus], valid)"""
    b = [int(x) for x in sf[:11]]
    n = num_aus_of(b[2])
    fields = [b[3] << 4 | b[4] >> 4, (b[4] & 15) << 8 | b[5], b[6] << 4 | b[7] >> 4, (b[7] & 15) << 8 | b[8],
              b[9] << 4 | b[10] >> 4]
    st = [HEADER_LEN[n]] + fields[:n - 1] + [len(sf)]
    return n, st, all(st[i + 1] - st[i] >= 3 for i in range(n))


def au_table_model(superframes, rsdims, ret=None):
    """(n, 110*rsdims) bytes [, n RS return values] -> n records of AU_DTYPE"""
    sfs = np.asarray(superframes, np.uint8).reshape(-1, 110 * rsdims)
    out = np.zeros(sfs.shape[0], AU_DTYPE)
    fire = fire_ok_model(sfs)
    for i, sf in enumerate(sfs):
        if ret is not None and ret[i] < 0:
            out[i]["status"] = AU_RS_FAILED
            continue
        n, st, valid = parse_header(sf)
        rec = out[i]
        rec["status"] = AU_OK if valid else AU_BAD_HEADER
        rec["num_aus"], rec["param"], rec["fire_ok"] = n, sf[2], fire[i]
        rec["au_start"][:n + 1] = st
        if valid:
            raw = sf.tobytes()
            rec["crc_ok"] = sum(1 << k for k in range(n)
                                if crc16_au(raw[st[k]:st[k + 1] - 2]) == (raw[st[k + 1] - 2] << 8 | raw[st[k + 1] - 1]))
    return out


# ---- the builder ----------------------------------------------------------------------------------------------------

def make_superframe(rng, rsdims, param, starts):
    """a superframe of 110*rsdims bytes: byte 2 = param, au_start[1 .. num_aus-1] = starts (padding bits 0, the
    header bytes a smaller num_aus leaves unused are AU bytes), random payloads, every AU's CRC where the header is
    valid, and the fire code"""
    L = 110 * rsdims
    n = num_aus_of(param)
    assert len(starts) == n - 1 and all(0 <= s < 4096 for s in starts)
    sf = rng.integers(0, 256, L, dtype=np.uint8)
    sf[2] = param
    bits = 0
    for s in starts:
        bits = bits << 12 | int(s)
    nb = 12 * (n - 1)
    if nb % 8:
        bits, nb = bits << 4, nb + 4
    sf[3:3 + nb // 8] = list(bits.to_bytes(nb // 8, "big"))
    st = [HEADER_LEN[n]] + [int(s) for s in starts] + [L]
    if all(st[i + 1] - st[i] >= 3 for i in range(n)):
        for i in range(n):
            c = crc16_au(sf[st[i]:st[i + 1] - 2].tobytes())
            sf[st[i + 1] - 2], sf[st[i + 1] - 1] = c >> 8, c & 0xFF
    return with_fire_code(sf)


def random_starts(rng, rsdims, n):
    """au_start[1 .. n-1] of a valid header: random cuts at least 3 bytes apart"""
    L = 110 * rsdims
    lo, hi = HEADER_LEN[n] + 3, min(L - 3, 4095)
    while True:
        st = sorted(int(x) for x in rng.integers(lo, hi + 1, n - 1))
        full = [HEADER_LEN[n]] + st + [L]
        if all(full[i + 1] - full[i] >= 3 for i in range(n)):
            return st


def host_table(V, sfs, rsdims):
    return np.array([V.dabplus_aus_host(sf, rsdims) for sf in np.asarray(sfs, np.uint8).reshape(-1, 110 * rsdims)], AU_DTYPE)


def same(a, b):
    """records compared byte for byte"""
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---- the model against the definition -------------------------------------------------------------------------------

def test_crc_table_equals_the_bit_loop():
    assert crc16_au(b"123456789") == 0xD64E
    rng = np.random.default_rng(1)
    for n in (1, 2, 3, 30, 64, 65, 127, 128, 500):
        au = rng.integers(0, 256, n, dtype=np.uint8)
        assert crc16_au(au) == crc16_genibus(au)


def test_known_header():
    sf = np.zeros(110 * 24, np.uint8)
    sf[3:8] = [0x12, 0x34, 0x56, 0x78, 0x90]
    n, st, valid = parse_header(sf)
    assert n == 4 and st == [8, 0x123, 0x456, 0x789, 2640] and valid
    rec = au_table_model(sf[None], 24)[0]
    assert rec["status"] == AU_OK and rec["num_aus"] == 4 and rec["param"] == 0
    assert rec["au_start"].tolist() == [8, 0x123, 0x456, 0x789, 2640, 0, 0]
    # the same starts in a 110-byte superframe leave it: a bad header, reported as parsed
    rec = au_table_model(sf[None, :110], 1)[0]
    assert rec["status"] == AU_BAD_HEADER and rec["au_start"].tolist() == [8, 0x123, 0x456, 0x789, 110, 0, 0]
    assert rec["crc_ok"] == 0


def test_every_num_aus_and_the_builder():
    rng = np.random.default_rng(2)
    for param, n in ((0x20, 2), (0x60, 3), (0x00, 4), (0x40, 6), (0xBF, 2), (0xFF, 3), (0x9F, 4), (0xDF, 6)):
        assert num_aus_of(param) == n
        for rsdims in (1, 24, 48):
            st = random_starts(rng, rsdims, n)
            sf = make_superframe(rng, rsdims, param, st)
            rec = au_table_model(sf[None], rsdims)[0]
            assert rec["status"] == AU_OK and rec["num_aus"] == n and rec["param"] == param and rec["fire_ok"] == 1
            assert rec["au_start"].tolist() == ([HEADER_LEN[n]] + st + [110 * rsdims] + [0] * 6)[:7]
            assert rec["crc_ok"] == (1 << n) - 1 and rec["reserved"] == 0
            full = rec["au_start"][:n + 1].tolist()
            for k in range(n):  # the bit loop agrees on every AU
                au = sf[full[k]:full[k + 1]]
                assert crc16_genibus(au[:-2]) == (int(au[-2]) << 8 | int(au[-1]))
            # a flipped payload bit clears exactly that AU's flag; a flipped header bit clears the fire flag
            k = int(rng.integers(0, n))
            bad = sf.copy()
            bad[full[k]] ^= 0x10
            assert au_table_model(bad[None], rsdims)[0]["crc_ok"] == ((1 << n) - 1) ^ (1 << k)
            bad = sf.copy()
            bad[2] ^= 0x01
            assert au_table_model(bad[None], rsdims)[0]["fire_ok"] == 0


def test_gated_records_are_zero():
    rng = np.random.default_rng(3)
    sfs = np.stack([make_superframe(rng, 2, 0x00, random_starts(rng, 2, 4)) for _ in range(3)])
    t = au_table_model(sfs, 2, ret=np.array([0, -1, 5]))
    assert t["status"].tolist() == [AU_OK, AU_RS_FAILED, AU_OK]
    assert t[1].tobytes() == bytes([AU_RS_FAILED]) + bytes(19)
    assert same(t[[0, 2]], au_table_model(sfs[[0, 2]], 2))


# ---- the library's host form ----------------------------------------------------------------------------------------

def test_au_record_layout(V):
    assert V.AU_DTYPE == AU_DTYPE and AU_DTYPE.itemsize == 20
    assert (V.AU_OK, V.AU_RS_FAILED, V.AU_BAD_HEADER) == (AU_OK, AU_RS_FAILED, AU_BAD_HEADER)
    assert [AU_DTYPE.fields[k][1] for k in ("status", "num_aus", "param", "crc_ok", "au_start", "fire_ok", "reserved")] == \
        [0, 1, 2, 3, 4, 18, 19]


@pytest.mark.parametrize("rsdims", [1, 2, 24, 37, 48])
def test_host_valid_superframes(V, rsdims):
    rng = np.random.default_rng(10 + rsdims)
    sfs = []
    for n in (2, 3, 4, 6):
        for _ in range(6):
            sf = make_superframe(rng, rsdims, PARAM[n] | int(rng.integers(0, 32)) | (int(rng.integers(0, 2)) << 7),
                                 random_starts(rng, rsdims, n))
            sfs.append(sf)
            hurt = sf.copy()  # one damaged byte anywhere behind the header
            hurt[int(rng.integers(11, 110 * rsdims))] ^= 1 << int(rng.integers(0, 8))
            sfs.append(hurt)
    want = au_table_model(np.stack(sfs), rsdims)
    assert (want["status"] == AU_OK).all() and (want["crc_ok"][::2] == (1 << want["num_aus"][::2]) - 1).all()
    assert (want["crc_ok"][1::2] != (1 << want["num_aus"][1::2]) - 1).all()
    assert same(host_table(V, sfs, rsdims), want)


@pytest.mark.parametrize("rsdims", [1, 2, 24, 37, 48])
def test_host_header_rule_violations(V, rsdims):
    """each way of breaking au_start[n+1] - au_start[n] >= 3: a start equal to or below its predecessor, within 2 of
    it, at or past L - 2, and a first start below the header length + 3"""
    rng = np.random.default_rng(20 + rsdims)
    L = 110 * rsdims
    sfs, nbad = [], 0
    for n in (2, 3, 4, 6):
        good = random_starts(rng, rsdims, n)
        cases = [good]
        for k in range(n - 1):
            pred = HEADER_LEN[n] if k == 0 else good[k - 1]
            for v in (pred, pred - 1, 0, pred + 1, pred + 2, pred + 3):
                cases.append(good[:k] + [max(v, 0)] + good[k + 1:])
        for v in (L - 3, L - 2, L - 1, L, L + 5, 4095):
            if v < 4096:
                cases.append(good[:-1] + [v])
        for v in range(HEADER_LEN[n] + 3):
            cases.append([v] + good[1:])
        for st in cases:
            sfs.append(make_superframe(rng, rsdims, PARAM[n], st))
    want = au_table_model(np.stack(sfs), rsdims)
    nbad = int((want["status"] == AU_BAD_HEADER).sum())
    assert nbad >= 40 and int((want["status"] == AU_OK).sum()) >= 4
    assert (want["crc_ok"][want["status"] == AU_BAD_HEADER] == 0).all() and (want["fire_ok"] == 1).all()
    assert same(host_table(V, sfs, rsdims), want)


@pytest.mark.parametrize("rsdims", [1, 2, 24, 37, 48])
def test_host_random_bytes(V, rsdims):
    rng = np.random.default_rng(30 + rsdims)
    sfs = rng.integers(0, 256, (200, 110 * rsdims), dtype=np.uint8)
    sfs[100:, 3:11] &= 0x0F if rsdims < 3 else 0x7F  # smaller fields: some headers hold
    want = au_table_model(sfs, rsdims)
    assert same(host_table(V, sfs, rsdims), want)
    assert (want["status"] == AU_BAD_HEADER).any()


def test_host_argument_errors(V):
    import ctypes as C
    L = V.lib()
    sf = np.zeros(110 * 48, np.uint8)
    out = np.full(2, 0xEE, np.uint8).repeat(20).view(AU_DTYPE)
    p, o = sf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for args in ((None, 1, o), (p, 1, None), (p, 0, o), (p, 49, o), (p, 1 << 31, o)):
        assert L.vit_dabplus_aus_host(*args) == 1  # VIT_ERR_ARG
        assert "vit_dabplus_aus_host" in V.last_error()
    assert (out.view(np.uint8) == 0xEE).all()
    assert L.vit_dabplus_aus_host(p, 48, o) == 0
    assert (out[1:].view(np.uint8) == 0xEE).all() and out[0]["reserved"] == 0  # one record, written completely
    with pytest.raises(ValueError):
        V.dabplus_aus_host(sf, 47)


NEW_EXPORTS = ("vit_dabplus_aus_dev", "vit_dabplus_aus_host", "vit_fire_code_dev")


def test_au_exports(V):
    out = subprocess.check_output(["nm", "-D", "--defined-only", V.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in NEW_EXPORTS:
        assert name in exported and name in V.EXPORTS


def test_au_calls_fail_loudly(V):
    """without a device: VIT_ERR_NO_DEVICE; with one, null buffers are VIT_ERR_ARG - nothing is launched either way"""
    import torch
    want = 1 if torch.cuda.is_available() else 2  # VIT_ERR_ARG / VIT_ERR_NO_DEVICE
    L = V.lib()
    assert L.vit_dabplus_aus_dev(None, 2640, 24, 4, None, None, None) == want
    assert L.vit_fire_code_dev(None, 576, 4, None, None) == want
    if want == 2:
        assert "gfx950" in V.last_error()
