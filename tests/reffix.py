"""Seeded inputs of the reference fixtures (tests/golden/reference_*.npy), shared by the generator
(tests/golden/make_reference_golden.py), the CPU tests (tests/test_ref_parity.py) and the GPU test
(tests/test_gpu_reference.py).  Pure numpy: neither the oracle nor oracle/_ref is needed to rebuild an input, and
numpy's own random generators are not used (their streams may change between versions).

Byte stream: x ^= x << 13; x ^= x >> 7; x ^= x << 17 on 64 bits, byte = (x >> 11) & 255 - the SURVEY KAT generator,
which oracle.uniform_symbols() also implements in C.
"""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DECODER_NPY = os.path.join(GOLD, "reference_decoder.npy")
RS_NPY = os.path.join(GOLD, "reference_rs.npy")
PROVENANCE_JSON = os.path.join(GOLD, "reference_provenance.json")
M64 = (1 << 64) - 1

# ---- decoder fixtures: every even framebits 2 ... 9216, two families --------------------------------------------
LENGTHS = list(range(2, 9217, 2))
# columns of reference_decoder.npy (uint64, one row per entry of LENGTHS): FNV-1a-64 of the inputs, then of the reference's
# output for {soft, hard} x {RENORMALIZE_THRESHOLD 150 (`> 150`), 149 (`>= 150`)}
COLS = ("in_soft", "in_hard", "soft_gt", "soft_ge", "hard_gt", "hard_ge")


def soft_seed(fb):
    """soft family: the stream's bytes as they come"""
    return (fb * 0x9E3779B97F4A7C15 + 0x0123456789ABCDEF) & M64


def hard_seed(fb):
    """hard family: 255 where the stream's byte has bit 7 set, else 0"""
    return (fb * 0xD1B54A32D192ED03 + 0xFEDCBA9876543210) & M64


def sym_len(fb):
    return 4 * (fb + 6)


def xorshift_bytes(seeds, lengths):
    """one byte stream per seed, all advanced together (numpy over the streams) -> list of uint8 arrays"""
    seeds = np.asarray(seeds, np.uint64)
    lengths = np.asarray(lengths, np.int64)
    assert seeds.size == lengths.size and (seeds != 0).all()
    order = np.argsort(-lengths, kind="stable")
    st, ln = seeds[order].copy(), lengths[order]
    outs = [np.empty(int(n), np.uint8) for n in ln]
    a, b, c, d = np.uint64(13), np.uint64(7), np.uint64(17), np.uint64(11)
    pos, maxlen, chunk = 0, int(ln[0]) if ln.size else 0, 2048
    while pos < maxlen:
        act = int(np.count_nonzero(ln > pos))  # the longest streams come first
        steps = min(chunk, maxlen - pos)
        blk = np.empty((steps, act), np.uint8)
        s = st[:act]
        for i in range(steps):
            s ^= s << a
            s ^= s >> b
            s ^= s << c
            blk[i] = (s >> d).astype(np.uint8)
        blk = np.ascontiguousarray(blk.T)
        for r in range(act):
            n = min(steps, int(ln[r]) - pos)
            outs[r][pos:pos + n] = blk[r, :n]
        pos += steps
    res = [None] * len(outs)
    for k, r in enumerate(order):
        res[int(r)] = outs[k]
    return res


def decoder_inputs(lengths=None):
    """-> (soft, hard): two lists of uint8 symbol arrays, 4*(fb+6) bytes each, for the given lengths (default: all)"""
    lengths = LENGTHS if lengths is None else list(lengths)
    n = len(lengths)
    rows = xorshift_bytes([soft_seed(fb) for fb in lengths] + [hard_seed(fb) for fb in lengths],
                          [sym_len(fb) for fb in lengths] * 2)
    return rows[:n], [((r >> 7) * 255).astype(np.uint8) for r in rows[n:]]


def fnv1a64(a):
    """FNV-1a-64 of a byte array (numpy: 8 independent lanes would not be FNV, so plain Python over the bytes)"""
    h = 0xcbf29ce484222325
    for x in np.ascontiguousarray(a, np.uint8).tobytes():
        h = ((h ^ x) * 0x100000001b3) & M64
    return h


def fnv1a64_rows(rows):
    """FNV-1a-64 of every row of a list of byte arrays, all rows advanced together"""
    n = len(rows)
    ln = np.array([r.size for r in rows], np.int64)
    order = np.argsort(-ln, kind="stable")
    h = np.full(n, 0xcbf29ce484222325, np.uint64)
    prime = np.uint64(0x100000001b3)
    maxlen = int(ln.max()) if n else 0
    lns = ln[order]
    pos, chunk = 0, 512
    while pos < maxlen:
        act = int(np.count_nonzero(lns > pos))
        steps = min(chunk, maxlen - pos)
        blk = np.zeros((act, steps), np.uint8)
        for k in range(act):
            seg = rows[int(order[k])][pos:pos + steps]
            blk[k, :seg.size] = seg
        blk = np.ascontiguousarray(blk.T).astype(np.uint64)
        for i in range(steps):
            live = int(np.count_nonzero(lns[:act] > pos + i))
            h[:live] = (h[:live] ^ blk[i, :live]) * prime
        pos += steps
    out = np.empty(n, np.uint64)
    out[order] = h
    return out


# ---- GF(2^8) / 0x11D and the RS(120,110) encoder, independent of the oracle and of the harness -----------------
def _gf():
    alpha, log, x = np.zeros(255, np.int64), np.zeros(256, np.int64), 1
    for i in range(255):
        alpha[i], log[x] = x, i
        x <<= 1
        if x & 256:
            x ^= 0x11D
    mul = np.zeros((256, 256), np.uint8)
    nz = np.arange(1, 256)
    mul[1:, 1:] = alpha[(log[nz][:, None] + log[nz][None, :]) % 255]
    return alpha, log, mul


ALPHA, LOG, MUL = _gf()


def _generator():
    g = [1]  # g(x) = prod_{i=0..9} (x + alpha^i), lowest coefficient first
    for i in range(10):
        ng = [0] * (len(g) + 1)
        for j, c in enumerate(g):
            ng[j + 1] ^= c
            ng[j] ^= int(MUL[c, ALPHA[i]])
        g = ng
    return g


GEN = _generator()


def rs_parity(msg):
    """msg (..., 110) uint8 -> the ten parity bytes (..., 10) of the systematic shortened RS(255,245) code: LFSR division by g"""
    msg = np.asarray(msg, np.uint8)
    r = [np.zeros(msg.shape[:-1], np.uint8) for _ in range(10)]  # r[9] = highest coefficient
    for k in range(110):
        fb = msg[..., k] ^ r[9]
        r = [MUL[fb, GEN[0]]] + [r[i - 1] ^ MUL[fb, GEN[i]] for i in range(1, 10)]
    return np.stack(r[::-1], axis=-1)


def _padding_parity_table():
    """row pos: parity bytes of the FULL-LENGTH codeword whose only non-zero data symbol is 1 at position pos (0 = x^254)
    of the 135 virtual padding symbols.  The code is linear: for a symbol v multiply the row by v."""
    t = np.zeros((135, 10), np.uint8)
    for pos in range(135):
        r = [0] * 10
        for k in range(pos, 245):
            fb = (1 if k == pos else 0) ^ r[9]
            r = [int(MUL[fb, GEN[0]])] + [r[i - 1] ^ int(MUL[fb, GEN[i]]) for i in range(1, 10)]
        t[pos] = r[::-1]
    return t


PAD_PARITY = _padding_parity_table()

# ---- RS superframes ------------------------------------------------------------------------------------------------
RS_DIMS = (1, 2, 7, 12, 24, 48)
RS_NSF = 48  # superframes per RSDims in the committed fixture
RS_SENTINEL = 0xA5
_KIND_WEIGHT = np.array([0, 0, 0, 1, 2, 3, 4, 5, 5, 6, 7, 8, 9, 10, -1, -2])  # -1: a pure random column, -2: padding symbol
# columns of reference_rs.npy (uint64, RS_NSF rows per entry of RS_DIMS, in that order)
RS_COLS = ("rsdims", "ret_as_u64", "out_fnv", "in_fnv")


def rs_seed(rsdims, sf, salt=0):
    return (((rsdims << 32) | sf) * 0x9E3779B97F4A7C15 + 0x5151515151515151 + salt) & M64 or 1


def rs_superframes(rsdims, nsf=RS_NSF, salt=0):
    """-> (p (nsf, 120*rsdims) uint8, kind (nsf, rsdims) int: injected error weight, -1 random column, -2 padding symbol).
    One stream per superframe, 256 bytes per column: [0] kind, [1] padding position, [2] padding value, [8:128] sort keys
    of the error positions, [128:138] error values, [140:250] message.  Superframe sf: sf % 3 == 0 has at most five errors
    per column (no failure), sf % 3 == 1 the same plus eight errors in the first / a middle / the last column in turn,
    sf % 3 == 2 the free mix."""
    rows = xorshift_bytes([rs_seed(rsdims, s, salt) for s in range(nsf)], [256 * rsdims] * nsf)
    R = np.stack(rows).reshape(nsf, rsdims, 256)
    kind = _KIND_WEIGHT[R[..., 0] & 15].copy()
    sf = np.arange(nsf)
    tame = (sf % 3 != 2)[:, None]
    kind = np.where(tame & (kind > 5), 5, kind)
    kind = np.where(tame & (kind == -1), 0, kind)
    hit = np.flatnonzero(sf % 3 == 1)
    kind[hit, np.array([0, rsdims // 2, rsdims - 1])[(hit // 3) % 3]] = 8
    cw = np.concatenate([R[..., 140:250], rs_parity(R[..., 140:250])], axis=-1)  # (nsf, rsdims, 120)
    rank = np.argsort(np.argsort(R[..., 8:128], axis=-1, kind="stable"), axis=-1, kind="stable")  # position -> its order
    val = np.where(R[..., 128:138] == 0, 1, R[..., 128:138]).astype(np.uint8)
    for w in range(10):  # the w-th error goes to the position of rank w, in columns with more than w errors
        sel = (rank == w) & (kind > w)[..., None]
        cw ^= np.where(sel, val[..., w][..., None], 0).astype(np.uint8)
    rnd = kind == -1
    cw[rnd] = R[..., 8:128][rnd]
    pad = kind == -2
    pv = np.where(R[..., 2] == 0, 1, R[..., 2]).astype(np.uint8)
    padpar = MUL[pv[..., None], PAD_PARITY[R[..., 1] % 135]]
    cw[..., 110:] ^= np.where(pad[..., None], padpar, 0).astype(np.uint8)
    p = np.ascontiguousarray(cw.transpose(0, 2, 1)).reshape(nsf, 120 * rsdims)  # byte k of column j at k*rsdims + j
    return p, kind
