"""CPU: packet mode (include/viterbi_amd.h, "Packet mode") - the numpy model of the three device calls, the builders of
packets and FEC frames (tests/test_gpu_packet.py imports both), and the host twin vit_packet_fec_frame_host against the
model.

The model's RS(204,188) decoder takes another route than the library's: the key equation by Euclid's algorithm, roots
counted over all 255 positions, error values from the Vandermonde system of the found positions, and the result accepted
only if all sixteen syndromes of the corrected row vanish.  The constants of the format stand once, below."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from reffix import ALPHA, LOG, MUL  # noqa: E402

# ---- the format (the library's: csrc/vit_packet_fmt.h) ------------------------------------------------------------------
SLOT = 24
FEC_DATA_SLOTS, FEC_PACKETS = 94, 9
FEC_SLOTS = FEC_DATA_SLOTS + FEC_PACKETS          # 103
FEC_FRAME_BYTES = FEC_SLOTS * SLOT                # 2472
FEC_DATA_BYTES = FEC_DATA_SLOTS * SLOT            # 2256
FEC_PARITY_PER_PACKET = 22
ADDR_FEC, ADDR_PADDING = 1022, 0
ROWS, COLS, NPAR = 12, 188, 16
NCODE = COLS + NPAR                               # 204
TCORR = NPAR // 2

FEC_REC_DTYPE = np.dtype([("nerr", "i1", (12,)), ("hdr_ok", "<u2"), ("status", "u1"), ("reserved", "u1")])
PACKET_REC_DTYPE = np.dtype([("kind", "u1"), ("crc_ok", "u1"), ("nslots", "u1"), ("flags", "u1"), ("address", "<u2"),
                             ("useful", "u1"), ("reserved", "u1")])
PKT_CONT, PKT_DATA, PKT_PADDING, PKT_FEC, PKT_OVERRUN = 0, 1, 2, 3, 4


def fec_hdr(c):
    return (c << 2 | ADDR_FEC >> 8, ADDR_FEC & 255)


def _fec_index():
    """IDX[r, k] = the frame byte of codeword position k of row r"""
    idx = np.zeros((ROWS, NCODE), np.int64)
    for r in range(ROWS):
        for k in range(COLS):
            idx[r, k] = ROWS * k + r
        for j in range(NPAR):
            m = ROWS * j + r
            idx[r, COLS + j] = FEC_DATA_BYTES + SLOT * (m // FEC_PARITY_PER_PACKET) + 2 + m % FEC_PARITY_PER_PACKET
    return idx


IDX = _fec_index()
MULL = MUL.tolist()
AL = [int(x) for x in ALPHA]
LG = [int(x) for x in LOG]


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- GF(2^8) polynomials, lowest coefficient first ------------------------------------------------------------------------
def ginv(x):
    return AL[(255 - LG[x]) % 255]


def pdeg(p):
    d = len(p) - 1
    while d >= 0 and p[d] == 0:
        d -= 1
    return d


def padd(a, b):
    n = max(len(a), len(b))
    return [(a[i] if i < len(a) else 0) ^ (b[i] if i < len(b) else 0) for i in range(n)]


def pmul(a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] ^= MULL[x][y]
    return out


def pdivmod(a, b):
    a = list(a)
    db = pdeg(b)
    inv = ginv(b[db])
    q = [0] * max(1, len(a))
    for d in range(pdeg(a), db - 1, -1):
        if a[d]:
            f = MULL[a[d]][inv]
            q[d - db] = f
            for j in range(db + 1):
                a[d - db + j] ^= MULL[f][b[j]]
    return q, a


def peval(p, x):
    v = 0
    for c in reversed(p):
        v = MULL[v][x] ^ c
    return v


def gsolve(A, y):
    """A x = y over GF(2^8), A square (lists); None if singular"""
    n = len(A)
    M = [list(A[i]) + [y[i]] for i in range(n)]
    for c in range(n):
        piv = next((r for r in range(c, n) if M[r][c]), None)
        if piv is None:
            return None
        M[c], M[piv] = M[piv], M[c]
        inv = ginv(M[c][c])
        M[c] = [MULL[v][inv] for v in M[c]]
        for r in range(n):
            if r != c and M[r][c]:
                f = M[r][c]
                M[r] = [M[r][j] ^ MULL[f][M[c][j]] for j in range(n + 1)]
    return [M[i][n] for i in range(n)]


def _generator16():
    g = [1]
    for i in range(NPAR):
        g = pmul(g, [AL[i], 1])
    return g


GEN16 = _generator16()
# VAND[i, k] = alpha^(i * (203 - k)): S_i = XOR_k MUL[cw[k], VAND[i, k]]
VAND = ALPHA[(np.arange(NPAR)[:, None] * (NCODE - 1 - np.arange(NCODE))[None, :]) % 255].astype(np.uint8)


def syndromes(cw):
    """cw (..., 204) -> (..., 16)"""
    cw = np.asarray(cw, np.uint8)
    return np.bitwise_xor.reduce(MUL[cw[..., None, :], VAND], axis=-1)


def rs_parity16(data):
    """data (..., 188) uint8 -> the sixteen parity bytes (..., 16), parity byte 15 the constant term: division by g(x)"""
    data = np.asarray(data, np.uint8)
    r = [np.zeros(data.shape[:-1], np.uint8) for _ in range(NPAR)]  # r[15] = highest coefficient
    for k in range(COLS):
        fb = data[..., k] ^ r[NPAR - 1]
        r = [MUL[fb, GEN16[0]]] + [r[i - 1] ^ MUL[fb, GEN16[i]] for i in range(1, NPAR)]
    return np.stack(r[::-1], axis=-1)


def encode_rows(data):
    data = np.asarray(data, np.uint8)
    return np.concatenate([data, rs_parity16(data)], axis=-1)


def decode_row_model(cw):
    """one row of 204 bytes -> (the row after decoding, nerr)"""
    cw = np.asarray(cw, np.uint8)
    S = [int(x) for x in syndromes(cw)]
    if not any(S):
        return cw.copy(), 0
    # Euclid on x^16 and S(x) until the remainder's degree is below 8
    r0, r1 = [0] * NPAR + [1], S
    t0, t1 = [0], [1]
    while pdeg(r1) >= TCORR:
        q, rem = pdivmod(r0, r1)
        r0, r1 = r1, rem
        t0, t1 = t1, padd(t0, pmul(q, t1))
    L = pdeg(t1)
    if L < 1 or L > TCORR or t1[0] == 0:
        return cw.copy(), -1
    lam = t1[:L + 1]
    degs = [d for d in range(255) if peval(lam, AL[(255 - d) % 255]) == 0]  # X = alpha^d over ALL 255 positions
    if len(degs) != L or max(degs) >= NCODE:
        return cw.copy(), -1
    vals = gsolve([[AL[(i * d) % 255] for d in degs] for i in range(L)], S[:L])
    if vals is None or not all(vals):
        return cw.copy(), -1
    out = cw.copy()
    for d, v in zip(degs, vals):
        out[NCODE - 1 - d] ^= v
    if syndromes(out).any():
        return cw.copy(), -1
    return out, L


def fec_frame_model(frame):
    """one FEC frame of 2472 bytes -> (the decoded frame, its FEC_REC_DTYPE record)"""
    frame = np.array(frame, np.uint8)
    rec = np.zeros(1, FEC_REC_DTYPE)
    for r in range(ROWS):
        row, ne = decode_row_model(frame[IDX[r]])
        frame[IDX[r]] = row
        rec["nerr"][0, r] = ne
    for c in range(FEC_PACKETS):
        if tuple(frame[FEC_DATA_BYTES + SLOT * c:FEC_DATA_BYTES + SLOT * c + 2]) == fec_hdr(c):
            rec["hdr_ok"][0] |= 1 << c
    rec["status"][0] = 1 if (rec["nerr"][0] < 0).any() else 0
    return frame, rec[0]


def fec_stream_model(stream, phase):
    """the stream after vit_packet_fec_dev and the records of its whole frames"""
    stream = np.array(stream, np.uint8)
    nslots = stream.size // SLOT
    nfec = (nslots - phase) // FEC_SLOTS if nslots > phase else 0
    recs = np.zeros(nfec, FEC_REC_DTYPE)
    for k in range(nfec):
        o = SLOT * (phase + FEC_SLOTS * k)
        stream[o:o + FEC_FRAME_BYTES], recs[k] = fec_frame_model(stream[o:o + FEC_FRAME_BYTES])
    return stream, recs


def build_fec_frame(app):
    """2256 bytes of application data -> the FEC frame of 2472 bytes (padding 0)"""
    app = np.asarray(app, np.uint8).reshape(FEC_DATA_BYTES)
    frame = np.zeros(FEC_FRAME_BYTES, np.uint8)
    frame[:FEC_DATA_BYTES] = app
    rows = encode_rows(app[IDX[:, :COLS]])
    frame[IDX] = rows
    for c in range(FEC_PACKETS):
        frame[FEC_DATA_BYTES + SLOT * c:FEC_DATA_BYTES + SLOT * c + 2] = fec_hdr(c)
    return frame


def sync_model(stream):
    stream = np.asarray(stream, np.uint8)
    nslots = stream.size // SLOT
    score = np.zeros(FEC_SLOTS, np.uint32)
    for p in range(FEC_SLOTS):
        for i in range(nslots):
            m = (i - p) % FEC_SLOTS
            if m >= FEC_DATA_SLOTS and tuple(stream[SLOT * i:SLOT * i + 2]) == fec_hdr(m - FEC_DATA_SLOTS):
                score[p] += 1
    return score


# ---- packets --------------------------------------------------------------------------------------------------------------
def _crc_table():
    t = []
    for b in range(256):
        r = b << 8
        for _ in range(8):
            r = ((r << 1) ^ 0x1021) & 0xFFFF if r & 0x8000 else (r << 1) & 0xFFFF
        t.append(r)
    return t


CRC_TABLE = _crc_table()


def crc16(data):
    """CRC-16 0x1021, preset 0xFFFF, MSB first, complemented"""
    r = 0xFFFF
    for b in bytes(bytearray(data)):
        r = ((r << 8) & 0xFFFF) ^ CRC_TABLE[(r >> 8) ^ b]
    return r ^ 0xFFFF


assert crc16(b"123456789") == 0xD64E


def make_packet(rng, nslots, address, cont=0, fl=0, command=0, useful=None):
    """a packet of nslots slots with random payload and a good CRC"""
    n = SLOT * nslots
    p = rng.integers(0, 256, n, dtype=np.uint8)
    useful = int(rng.integers(0, min(n - 5, 127) + 1)) if useful is None else useful
    p[0] = (nslots - 1) << 6 | cont << 4 | fl << 2 | address >> 8
    p[1] = address & 255
    p[2] = command << 7 | useful
    c = crc16(p[:n - 2])
    p[n - 2], p[n - 1] = c >> 8, c & 255
    return p


def random_packets(rng, lengths):
    """packets of the given slot counts with random data addresses and header fields, back to back"""
    out = []
    for n in lengths:
        addr = int(rng.integers(1, 1022))
        out.append(make_packet(rng, n, addr, int(rng.integers(0, 4)), int(rng.integers(0, 4)), int(rng.integers(0, 2))))
    return np.concatenate(out)


def packets_model(stream, framebytes):
    stream = np.asarray(stream, np.uint8)
    S = framebytes // SLOT
    nframes = stream.size // framebytes
    rec = np.zeros(nframes * S, PACKET_REC_DTYPE)
    for f in range(nframes):
        fr = stream[f * framebytes:(f + 1) * framebytes]
        i = 0
        while i < S:
            b0, b1, b2 = (int(x) for x in fr[SLOT * i:SLOT * i + 3])
            addr = (b0 & 3) << 8 | b1
            n = 1 if addr == ADDR_FEC else (b0 >> 6) + 1
            if i + n > S:
                rec["kind"][f * S + i:(f + 1) * S] = PKT_OVERRUN
                break
            r = rec[f * S + i:f * S + i + 1]
            if addr == ADDR_FEC:
                r["kind"], r["nslots"], r["flags"], r["address"] = PKT_FEC, 1, (b0 >> 2) & 15, addr
            else:
                pk = fr[SLOT * i:SLOT * (i + n)]
                r["kind"] = PKT_PADDING if addr == ADDR_PADDING else PKT_DATA
                r["crc_ok"] = 1 if crc16(pk[:-2]) == (int(pk[-2]) << 8 | int(pk[-1])) else 0
                r["nslots"] = n
                r["flags"] = ((b0 >> 4) & 3) | ((b0 >> 2) & 3) << 2 | (b2 >> 7) << 4
                r["address"] = addr
                r["useful"] = b2 & 0x7F
            i += n
    return rec


def length_mixes(total):
    """every sequence of packet lengths 1 ... 4 that fills `total` slots exactly (total small)"""
    if total == 0:
        return [[]]
    return [[n] + rest for n in range(1, min(4, total) + 1) for rest in length_mixes(total - n)]


# ---- directed rows --------------------------------------------------------------------------------------------------------
def low_weight_word(degs, first=1):
    """the word of the full-length code with support on the 17 distinct degrees `degs` (0 ... 254) and value `first` at
    degs[0]: {degree: value}; the other sixteen values follow from the sixteen syndrome equations"""
    assert len(degs) == NPAR + 1 and len(set(degs)) == NPAR + 1
    A = [[AL[(i * d) % 255] for d in degs[1:]] for i in range(NPAR)]
    y = [MULL[first][AL[(i * degs[0]) % 255]] for i in range(NPAR)]
    vals = gsolve(A, y)
    assert vals is not None and all(vals)
    return dict(zip(degs, [first] + vals))


def miscorrection_row(rng):
    """(received, expected): a codeword A plus 9 of the 17 bytes of a weight-17 codeword w -> A + w, nerr 8"""
    A = encode_rows(rng.integers(0, 256, COLS, dtype=np.uint8))
    degs = [int(x) for x in rng.permutation(NCODE)[:NPAR + 1]]
    w = low_weight_word(degs, int(rng.integers(1, 256)))
    got, want = A.copy(), A.copy()
    for n, d in enumerate(degs):
        want[NCODE - 1 - d] ^= w[d]
        if n < 9:
            got[NCODE - 1 - d] ^= w[d]
    return got, want


def padding_root_row(rng):
    """a codeword A plus 9 real bytes of a weight-17 word with one byte among the 51 virtual positions: the nearest
    full-length codeword is 8 away, one of the differences in the padding -> -1, unchanged"""
    A = encode_rows(rng.integers(0, 256, COLS, dtype=np.uint8))
    real = [int(x) for x in rng.permutation(NCODE)[:NPAR]]
    degs = real[:9] + [int(rng.integers(NCODE, 255))] + real[9:]
    w = low_weight_word(degs, int(rng.integers(1, 256)))
    got = A.copy()
    for d in degs[:9]:
        got[NCODE - 1 - d] ^= w[d]
    return got


def plant(rng, row, positions):
    row = row.copy()
    for k in positions:
        row[k] ^= int(rng.integers(1, 256))
    return row


# ---- tests ----------------------------------------------------------------------------------------------------------------
def test_encoder_rows_have_zero_syndromes():
    rng = np.random.default_rng(1)
    rows = encode_rows(rng.integers(0, 256, (64, COLS), dtype=np.uint8))
    assert not syndromes(rows).any()
    assert syndromes(plant(rng, rows[0], [5])).any()
    frame = build_fec_frame(rng.integers(0, 256, FEC_DATA_BYTES, dtype=np.uint8))
    assert not syndromes(frame[IDX]).any()
    assert not frame[-6:].any() and tuple(frame[FEC_DATA_BYTES + SLOT * 8:][:2]) == (8 << 2 | 3, 0xFE)


def planted_rows(rng):
    """rows with 0 ... 8 errors in data, parity and both, positions 0, 187, 188 and 203 among them: (row, codeword, n)"""
    out = []
    for n in range(0, 9):
        for where in ("data", "parity", "both", "edges"):
            cw = encode_rows(rng.integers(0, 256, COLS, dtype=np.uint8))
            if where == "data":
                pos = rng.permutation(COLS)[:n]
            elif where == "parity":
                pos = COLS + rng.permutation(NPAR)[:n]
            elif where == "both":
                pos = np.concatenate([rng.permutation(COLS)[:n // 2], COLS + rng.permutation(NPAR)[:n - n // 2]])
            else:
                pos = np.array([0, 187, 188, 203] + [int(x) for x in 1 + rng.permutation(186)[:4]])[:n]
            out.append((plant(rng, cw, [int(x) for x in pos]), cw, n))
    return out


def test_model_corrects_planted_errors():
    rng = np.random.default_rng(2)
    for row, cw, n in planted_rows(rng):
        got, ne = decode_row_model(row)
        assert ne == n and np.array_equal(got, cw)


def test_model_directed_miscorrection_and_padding_root():
    rng = np.random.default_rng(3)
    for _ in range(4):
        row, want = miscorrection_row(rng)
        got, ne = decode_row_model(row)
        assert ne == 8 and np.array_equal(got, want) and not syndromes(want).any()
        row = padding_root_row(rng)
        got, ne = decode_row_model(row)
        assert ne == -1 and np.array_equal(got, row)


def frame_of_rows(rng, rows):
    """an FEC frame whose first len(rows) rows are the given 204-byte rows, the others clean codewords"""
    frame = build_fec_frame(rng.integers(0, 256, FEC_DATA_BYTES, dtype=np.uint8))
    for r, row in enumerate(rows):
        frame[IDX[r]] = row
    return frame


def random_damaged_frame(rng, max_err=12):
    frame = build_fec_frame(rng.integers(0, 256, FEC_DATA_BYTES, dtype=np.uint8))
    for r in range(ROWS):
        n = int(rng.integers(0, max_err + 1))
        frame[IDX[r]] = plant(rng, frame[IDX[r]], [int(x) for x in rng.permutation(NCODE)[:n]])
    return frame


def check_host(V, frame):
    want, wrec = fec_frame_model(frame)
    got, grec = V.packet_fec_frame_host(frame)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert grec.tobytes() == wrec.tobytes(), (grec, wrec)
    return wrec


def test_host_twin_against_the_model(V):
    assert V.FEC_REC_DTYPE == FEC_REC_DTYPE and V.PACKET_REC_DTYPE == PACKET_REC_DTYPE
    rng = np.random.default_rng(4)
    rows = [r for r, _, _ in planted_rows(rng)]
    for k in range(0, len(rows), ROWS):
        rec = check_host(V, frame_of_rows(rng, rows[k:k + ROWS]))
        assert rec["status"] == 0
    directed = [miscorrection_row(rng)[0] for _ in range(6)] + [padding_root_row(rng) for _ in range(6)]
    rec = check_host(V, frame_of_rows(rng, directed))
    assert rec["nerr"].tolist() == [8] * 6 + [-1] * 6 and rec["status"] == 1
    seen = set()
    for _ in range(200):
        seen.update(check_host(V, random_damaged_frame(rng))["nerr"].tolist())
    assert seen == set(range(-1, 9))
    # headers and padding lie outside the code
    frame = random_damaged_frame(rng, 3)
    frame[FEC_DATA_BYTES] ^= 4
    frame[FEC_DATA_BYTES + SLOT * 8 + 1] ^= 1
    frame[-1] ^= 0x55
    rec = check_host(V, frame)
    assert rec["hdr_ok"] == 0x1FF ^ 1 ^ 0x100
    L = V.lib()
    assert L.vit_packet_fec_frame_host(None, None) == 1 and "vit_packet_fec_frame_host" in V.last_error()
    assert V.packet_fec_count(103, 0) == 1 and V.packet_fec_count(103, 1) == 0 and V.packet_fec_count(5, 9) == 0
    assert V.packet_fec_count(2 * 103 + 101, 102) == 1 and V.packet_fec_count(2 * 103 + 102, 102) == 2
    assert L.vit_packet_fec_count(10, 103) == -1 and L.vit_packet_fec_count(-1, 0) == -1


def build_stream(rng, nfec, phase, tail, framefill=None):
    """phase slots of packets, nfec FEC frames of random data packets, `tail` more slots -> stream bytes"""
    def fill(nsl):
        lengths = []
        while sum(lengths) < nsl:
            lengths.append(int(rng.integers(1, min(4, nsl - sum(lengths)) + 1)))
        return random_packets(rng, lengths) if lengths else np.zeros(0, np.uint8)
    parts = [fill(phase)]
    for _ in range(nfec):
        parts.append(build_fec_frame(fill(FEC_DATA_SLOTS)))
    parts.append(fill(tail))
    return np.concatenate(parts)


def build_framed_stream(rng, nfec, phase, nslots, S):
    """a stream of nslots slots in logical frames of S slots: nfec FEC frames from slot `phase`, every other slot filled
    with data packets that cross neither a logical frame's end nor an FEC packet"""
    assert nslots % S == 0 and phase + FEC_SLOTS * nfec <= nslots

    def is_fec(i):
        return i >= phase and (i - phase) // FEC_SLOTS < nfec and (i - phase) % FEC_SLOTS >= FEC_DATA_SLOTS
    st = np.zeros(nslots * SLOT, np.uint8)
    i = 0
    while i < nslots:
        if is_fec(i):
            i += 1
            continue
        room = 1
        while room < 4 and (i + room) % S and i + room < nslots and not is_fec(i + room):
            room += 1
        n = int(rng.integers(1, room + 1))
        st[SLOT * i:SLOT * (i + n)] = random_packets(rng, [n])
        i += n
    for k in range(nfec):
        o = SLOT * (phase + FEC_SLOTS * k)
        st[o:o + FEC_FRAME_BYTES] = build_fec_frame(st[o:o + FEC_DATA_BYTES])
    return st


def test_framed_stream_builder():
    rng = np.random.default_rng(7)
    st = build_framed_stream(rng, 2, 5, 216, 8)
    rec = packets_model(st, 192)
    assert not (rec["kind"] == PKT_OVERRUN).any() and int((rec["kind"] == PKT_FEC).sum()) == 18
    assert rec["crc_ok"][rec["kind"] == PKT_DATA].all() and int(np.argmax(sync_model(st))) == 5
    assert fec_stream_model(st, 5)[1]["nerr"].tolist() == [[0] * 12] * 2


def test_sync_scores_peak_at_the_planted_phase():
    rng = np.random.default_rng(5)
    for phase in (0, 50, 102):
        st = build_stream(rng, 3, phase, 40)
        score = sync_model(st)
        assert score[phase] == 27 and (np.delete(score, phase) < 27).all()


def test_packet_walk_model():
    rng = np.random.default_rng(6)
    for slots in (1, 2, 4, 5):
        for mix in length_mixes(slots):
            fr = random_packets(rng, mix)
            rec = packets_model(fr, SLOT * slots)
            starts = np.cumsum([0] + mix[:-1])
            assert rec["kind"][starts].tolist() == [PKT_DATA] * len(mix) and rec["nslots"][starts].tolist() == mix
            assert rec["crc_ok"][starts].all() and (np.delete(rec["kind"], starts) == PKT_CONT).all()
    for mix in ([1] * 48, [4] * 12, [1, 2, 3, 4] * 4 + [4, 4]):
        rec = packets_model(random_packets(rng, mix), 1152)
        assert int((rec["kind"] == PKT_DATA).sum()) == len(mix) and rec["crc_ok"].sum() == len(mix)
    # padding, FEC and overrun
    fr = np.concatenate([make_packet(rng, 2, ADDR_PADDING), np.zeros(SLOT, np.uint8), make_packet(rng, 3, 77)])
    fr[48:50] = fec_hdr(5)
    rec = packets_model(fr, 120)
    assert rec["kind"].tolist() == [PKT_PADDING, PKT_CONT, PKT_FEC, PKT_OVERRUN, PKT_OVERRUN]
    assert rec["crc_ok"].tolist() == [1, 0, 0, 0, 0] and rec["flags"][2] == 5 and rec["address"][2] == ADDR_FEC
    assert rec[3].tobytes() == bytes([PKT_OVERRUN]) + bytes(7)
    p = make_packet(rng, 1, 300, cont=2, fl=1, command=1, useful=17)
    r = packets_model(p, 24)[0]
    assert (r["flags"], r["address"], r["useful"], r["nslots"], r["crc_ok"]) == (2 | 1 << 2 | 16, 300, 17, 1, 1)
    p[7] ^= 1
    assert packets_model(p, 24)[0]["crc_ok"] == 0
