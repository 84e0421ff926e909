"""Syndrome-directed RS(120,110) columns: test inputs that choose the path a column takes through the decoder
(tests/test_rs_paths_host.py, tests/test_gpu_rs_paths.py, tests/golden/make_reference_golden.py).

The syndrome map of the shortened code is onto: for any ten byte positions the 10x10 Vandermonde system over GF(2^8) is
invertible, so a codeword with ten bytes adjusted has ANY chosen syndrome vector (column_with_syndromes).  A test can
therefore pick the locator Berlekamp-Massey will find - degree, root set, repeated or missing roots, roots in the 135
virtual padding positions - instead of waiting for "codeword plus random errors" to produce it.

Conventions (rschecksf.cpp): byte k of a column is the coefficient of x^(119-k); S_i = sum_k d_k alpha^(i*(119-k)),
i = 0..9; an error at byte k has locator X = alpha^(119-k) and is found by the Chien scan at index rt = k + 136
(X = alpha^(255-rt)); rt = 1..135 are the virtual padding symbols of RS(255,245).

Pure numpy: no oracle, no oracle/_ref, no numpy.random (the byte streams are reffix.xorshift_bytes), GF tables from reffix.
"""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import reffix  # noqa: E402
from reffix import ALPHA, LOG, MUL  # noqa: E402

RS_PATHS_NPY = os.path.join(reffix.GOLD, "reference_rs_paths.npy")
PAD = 135
NSYN = 10


# ---- seeded bytes ------------------------------------------------------------------------------------------------------
class Rng:
    """n seeded bytes per label (up to 4096 xorshift streams side by side), handed out in order"""

    def __init__(self, label, n):
        base = reffix.fnv1a64(np.frombuffer(label.encode(), np.uint8))
        k = min(4096, n)
        steps = -(-n // k)
        seeds = [((base + (i + 1) * 0x9E3779B97F4A7C15) & reffix.M64) or 1 for i in range(k)]
        self.buf = np.stack(reffix.xorshift_bytes(seeds, [steps + 8] * k))[:, 8:].T.reshape(-1)
        self.pos = 0

    def take(self, *shape):
        n = int(np.prod(shape))
        assert self.pos + n <= self.buf.size, "Rng: pool exhausted"
        out = self.buf[self.pos:self.pos + n].reshape(shape)
        self.pos += n
        return out

    def nonzero(self, *shape):
        v = self.take(*shape)
        return np.where(v == 0, 1, v).astype(np.uint8)

    def distinct(self, n, lo, hi, d):
        """n rows of d distinct integers from lo..hi (inclusive), in random order"""
        span = hi - lo + 1
        keys = self.take(n, span).astype(np.int64) * 256 + self.take(n, span)
        return lo + np.argsort(keys, axis=1, kind="stable")[:, :d]


# ---- GF(2^8) helpers ---------------------------------------------------------------------------------------------------
def gmul(a, b):
    return MUL[np.asarray(a, np.int64), np.asarray(b, np.int64)]


def ginv(a):
    a = np.asarray(a, np.int64)
    assert (a != 0).all()
    return ALPHA[(255 - LOG[a]) % 255].astype(np.uint8)


def locator_of(rt):
    """Chien index 1..255 -> X = alpha^(255 - rt)"""
    return ALPHA[(255 - np.asarray(rt, np.int64)) % 255].astype(np.uint8)


def geometric(Y, rt):
    """S_n = Y X^n, n = 0..9, X the locator of Chien index rt; Y != 0.  (...,) -> (..., 10)"""
    Y, rt = np.asarray(Y, np.int64), np.asarray(rt, np.int64)
    assert (Y != 0).all()
    n = np.arange(NSYN)
    return ALPHA[(LOG[Y][..., None] + n * ((255 - rt) % 255)[..., None]) % 255].astype(np.uint8)


def power_sums(Y, rt):
    """S_n = sum_j Y_j X_j^n: (n, d), (n, d) -> (n, 10)"""
    return np.bitwise_xor.reduce(geometric(Y, rt), axis=1)


def recurrence2(l1, l2, u0, u1):
    """u_n = l1 u_(n-1) + l2 u_(n-2): the sequences whose connection polynomial is 1 + l1 x + l2 x^2"""
    u = [np.asarray(u0, np.uint8), np.asarray(u1, np.uint8)]
    for _ in range(2, NSYN):
        u.append(gmul(l1, u[-1]) ^ gmul(l2, u[-2]))
    return np.stack(u, axis=-1)


def _no_solution():
    """the c for which y^2 + y = c has no solution (trace 1): 1 + l1 x + l2 x^2 with l2 / l1^2 = c is irreducible"""
    y = np.arange(256)
    have = np.zeros(256, bool)
    have[gmul(y, y) ^ y] = True
    return np.flatnonzero(~have)


NOSOL = _no_solution()


def horner_syndromes(words):
    """(n, 120) -> (n, 10): the reference's own sums, S_i = ((d_0 a^i + d_1) a^i + ...) + d_119"""
    words = np.asarray(words, np.uint8)
    ai = ALPHA[np.arange(NSYN)]
    s = np.repeat(words[:, :1], NSYN, axis=1)
    for k in range(1, 120):
        s = gmul(s, ai[None, :]) ^ words[:, k:k + 1]
    return s


@functools.lru_cache(maxsize=None)
def vandermonde_inverse(positions):
    """positions: ten distinct byte indices -> V^-1 (10, 10), V[i][j] = alpha^(i * (119 - positions[j]))"""
    assert len(positions) == NSYN and len(set(positions)) == NSYN and all(0 <= p < 120 for p in positions)
    n = NSYN
    a = [[int(ALPHA[(i * (119 - p)) % 255]) for p in positions] + [int(i == j) for j in range(n)] for i in range(n)]
    for c in range(n):  # Gauss-Jordan over GF(2^8)
        piv = next(r for r in range(c, n) if a[r][c])
        a[c], a[piv] = a[piv], a[c]
        inv = int(ginv(a[c][c]))
        a[c] = [int(MUL[inv, v]) for v in a[c]]
        for r in range(n):
            if r != c and a[r][c]:
                f = a[r][c]
                a[r] = [v ^ int(MUL[f, w]) for v, w in zip(a[r], a[c])]
    return np.array([row[n:] for row in a], np.uint8)


POSITION_SETS = (tuple(range(110, 120)),                          # parity rows only
                 (0, 7, 19, 33, 48, 54, 71, 86, 97, 109),           # message rows only
                 (3, 28, 55, 80, 104, 110, 112, 115, 117, 119))     # mixed


def column_with_syndromes(msg, s, positions):
    """msg (n, 110), s (n, 10) -> (n, 120): the codeword of msg with the bytes at `positions` XORed by V^-1 s"""
    msg, s = np.asarray(msg, np.uint8), np.asarray(s, np.uint8)
    vinv = vandermonde_inverse(tuple(positions))
    cw = np.concatenate([msg, reffix.rs_parity(msg)], axis=-1)
    for j, p in enumerate(positions):
        cw[:, p] ^= np.bitwise_xor.reduce(gmul(vinv[j][None, :], s), axis=1)
    return cw


# ---- the classes -------------------------------------------------------------------------------------------------------
class Klass:
    """words (n, 120); expect: the return value construction fixes, or None ("reference"); want: the whole decoded
    column where construction fixes that too (real_d, pad_d_m), else None; roots (n, d) where a root set was chosen"""

    def __init__(self, label, words, expect=None, want=None, roots=None, syn=None):
        self.label, self.words, self.expect, self.want, self.roots, self.syn = label, words, expect, want, roots, syn

    def __len__(self):
        return self.words.shape[0]


# root sets every run must contain (Chien indices), by class
_FIXED_ROOTS = {
    "real_1": [(136,), (255,), (137,), (254,)],
    "real_2": [(136, 255), (137, 138), (253, 254), (255, 254)],
    "real_3": [(253, 254, 255), (137, 138, 139), (136, 200, 255)],
    "real_4": [(137, 138, 139, 140), (136, 253, 254, 255), (252, 253, 254, 255), (141, 142, 143, 200)],
    "real_5": [(141, 142, 143, 144, 200), (136, 137, 138, 139, 140), (251, 252, 253, 254, 255)],
    "pad_1_1": [(1,), (135,), (2,), (134,)],
    "pad_2_1": [(1, 255), (135, 136), (1, 136)],
    "pad_2_2": [(1, 2), (1, 135), (134, 135)],
    "pad_3_1": [(1, 254, 255), (135, 136, 137)],
    "pad_3_2": [(1, 2, 255), (1, 135, 136)],
    "pad_3_3": [(1, 2, 3), (133, 134, 135)],
    "pad_4_1": [(1, 253, 254, 255)],
    "pad_4_2": [(1, 135, 136, 255)],
    "pad_4_3": [(1, 2, 3, 255)],
    "pad_4_4": [(1, 2, 3, 4), (132, 133, 134, 135)],
    "pad_5_1": [(1, 136, 253, 254, 255)],
    "pad_5_2": [(1, 2, 137, 138, 255)],
    "pad_5_3": [(1, 2, 3, 136, 255)],
    "pad_5_4": [(1, 2, 3, 4, 255), (132, 133, 134, 135, 136)],
    "pad_5_5": [(1, 2, 3, 4, 5), (131, 132, 133, 134, 135)],
}

N_DEFAULT = 96
N_SHORT = 256
N_DEG6_OK = 192
N_RANDOM = 24000


def _finish(label, rng, s, expect=None, roots=None, Y=None):
    """syndromes -> columns (the position sets in turn, random messages), with the decoded column where it is known"""
    n = s.shape[0]
    msg = rng.take(n, 110)
    words = np.empty((n, 120), np.uint8)
    for k, pos in enumerate(POSITION_SETS):
        words[k::3] = column_with_syndromes(msg[k::3], s[k::3], pos)
    want = None
    if Y is not None:  # a true error pattern of the full-length code: Forney returns Y_j at every root, padding included
        want = words.copy()
        for j in range(roots.shape[1]):
            real = roots[:, j] > PAD
            want[real, roots[real, j] - PAD - 1] ^= Y[real, j]
    return Klass(label, words, expect, want, roots, s)


def _root_class(label, d, m, n=N_DEFAULT):
    """d roots, m of them in the padding (Chien index 1..135), the others at bytes (136..255)"""
    rng = Rng(label, n * 1200)
    parts = []
    if m:
        parts.append(rng.distinct(n, 1, PAD, m))
    if d - m:
        parts.append(rng.distinct(n, PAD + 1, 255, d - m))
    roots = np.concatenate(parts, axis=1)
    for i, fixed in enumerate(_FIXED_ROOTS.get(label, [])):
        assert len(fixed) == d and sum(r <= PAD for r in fixed) == m, (label, fixed)
        roots[i] = fixed
    Y = rng.nonzero(n, d)
    return _finish(label, rng, power_sums(Y, roots), expect=d, roots=roots, Y=Y)


def _irreducible2(rng, n):
    l1 = rng.nonzero(n)
    c = NOSOL[rng.take(n).astype(np.int64) % NOSOL.size]
    return l1, gmul(c, gmul(l1, l1))


def _deg2_noroot(n=N_DEFAULT):
    rng = Rng("deg2_noroot", n * 200)
    l1, l2 = _irreducible2(rng, n)
    return _finish("deg2_noroot", rng, recurrence2(l1, l2, rng.nonzero(n), rng.take(n)), expect=-1)


def _deg2_double(n=N_DEFAULT):
    """1 + a^2 x^2 = (1 + a x)^2 with S_1 != a S_0, so that the shortest LFSR really has length 2"""
    rng = Rng("deg2_double", n * 200)
    a, u0 = rng.nonzero(n), rng.nonzero(n)
    return _finish("deg2_double", rng, recurrence2(np.zeros(n, np.uint8), gmul(a, a), u0, gmul(a, u0) ^ rng.nonzero(n)), expect=-1)


def _deg2_r0(n=N_DEFAULT):
    """two roots, one of them X = 1: its log is 0, the scan finds it at index 255"""
    rng = Rng("deg2_r0", n * 800)
    roots = np.concatenate([rng.distinct(n, 1, 254, 1), np.full((n, 1), 255)], axis=1)
    Y = rng.nonzero(n, 2)
    return _finish("deg2_r0", rng, power_sums(Y, roots), expect=2, roots=roots, Y=Y)


def _nosplit(d, n=N_DEFAULT):
    """even columns: an irreducible quadratic times d-2 distinct linear factors; odd columns: (1 + a x)^2 times d-2
    linear factors other than 1 + a x.  The summands' minimal polynomials are coprime, so the shortest LFSR of the sum
    is their product: degree d <= 5, unique, found by Berlekamp-Massey - and it has d-2 resp. d-1 roots."""
    label = "nosplit_%d" % d
    rng = Rng(label, n * 1200)
    roots = rng.distinct(n, 1, 255, d - 1)
    lin = power_sums(rng.nonzero(n, d - 2), roots[:, 1:])
    l1, l2 = _irreducible2(rng, n)
    quad = recurrence2(l1, l2, rng.nonzero(n), rng.take(n))
    a, u0 = locator_of(roots[:, 0]), rng.nonzero(n)
    rep = recurrence2(np.zeros(n, np.uint8), gmul(a, a), u0, gmul(a, u0) ^ rng.nonzero(n))
    odd = (np.arange(n) % 2 == 1)[:, None]
    return _finish(label, rng, lin ^ np.where(odd, rep, quad), expect=-1)


def _short(k, n=N_SHORT):
    """geometric syndromes with S_k changed.  k = 2, 3: the shortest LFSR is (k + 2, 1 + X x) and it is unique
    (2 (k + 2) <= 10; S(x)(1 + X x) = S_0 + e x^k (1 + X x) is coprime to 1 + X x, so nothing shorter exists): the
    reference returns 1 although the sequence is not one error's.  k >= 4: the reference decides."""
    label = "short_%d" % k
    rng = Rng(label, n * 200)
    s = geometric(rng.nonzero(n), 1 + rng.take(n).astype(np.int64) % 255).copy()
    s[:, k] ^= rng.nonzero(n)
    return _finish(label, rng, s, expect=1 if k <= 3 else None)


def _zero_s(i, n=N_DEFAULT):
    """power sums of 1..5 roots (padding or not) with S_i forced to 0"""
    label = "zero_s%d" % i
    rng = Rng(label, n * 1200)
    roots = rng.distinct(n, 1, 255, 5)
    Y = rng.nonzero(n, 5)
    d = 1 + np.arange(n) % 5
    s = np.bitwise_xor.reduce(np.where((np.arange(5)[None, :] < d[:, None])[..., None], geometric(Y, roots), 0), axis=1).astype(np.uint8)
    s[:, i] = 0
    return _finish(label, rng, s)


def _deg6_ok(n=N_DEG6_OK):
    """six distinct roots with a vanishing x^5 coefficient: five free (bytes), the sixth from e5 + X6 e4 = 0.  Syndromes
    (0, 0, 0, 0, 0, l6, then the recurrence): Berlekamp-Massey jumps to length 6 and ends in exactly this locator."""
    rng = Rng("deg6_ok", 4 * n * 1200)
    cand = 4 * n
    rt5 = rng.distinct(cand, PAD + 1, 255, 5)
    X = locator_of(rt5)
    e = np.zeros((cand, 7), np.uint8)  # elementary symmetric polynomials = the locator's coefficients
    e[:, 0] = 1
    for j in range(5):
        e[:, 1:] ^= gmul(e[:, :-1], X[:, j:j + 1])
    ok = e[:, 4] != 0
    x6 = np.where(ok, gmul(e[:, 5], ginv(np.where(ok, e[:, 4], 1))), 0)
    ok &= (x6 != 0) & (x6[:, None] != X).all(axis=1)
    rt5, e, x6 = rt5[ok][:n], e[ok][:n], x6[ok][:n]
    assert rt5.shape[0] == n, "deg6_ok: too few candidates"
    lam = e.copy()
    lam[:, 1:] ^= gmul(e[:, :-1], x6[:, None])
    assert (lam[:, 5] == 0).all() and (lam[:, 6] != 0).all()
    s = np.zeros((n, NSYN), np.uint8)
    s[:, 5] = lam[:, 6]
    for i in range(6, NSYN):
        for j in range(1, 5):
            s[:, i] ^= gmul(lam[:, j], s[:, i - j])
    roots = np.concatenate([rt5, ((255 - LOG[x6]) % 255)[:, None]], axis=1)
    roots[roots == 0] = 255
    return _finish("deg6_ok", rng, s, expect=6, roots=roots)


def _num1_zero(d, n=N_DEFAULT):
    """d roots at bytes, power sums with S_k changed by e (k = 0 for d = 1, else 1).  As in short_k the shortest LFSR is
    (k + d + 1, the true locator), unique since 2 (k + d + 1) <= 10, so the column returns d - but omega, cut at degree
    d - 1, is the true one plus e x^k lambda(x) cut likewise, and e is chosen so that it vanishes at the first root:
    Forney's num1 is 0 there and that byte stays unpatched (d = 1: S_0 = 0, nothing is patched at all)."""
    label = "num1_zero_%d" % d
    rng = Rng(label, 2 * n * 800)
    cand = 2 * n
    roots = rng.distinct(cand, PAD + 1, 255, d)
    Y = rng.nonzero(cand, d)
    X = locator_of(roots)
    lam = np.zeros((cand, d + 1), np.uint8)
    lam[:, 0] = 1
    for j in range(d):
        lam[:, 1:] ^= gmul(lam[:, :-1], X[:, j:j + 1])
    s = power_sums(Y, roots)
    k = 0 if d == 1 else 1
    z = ginv(X[:, 0])
    zp = [np.ones(cand, np.uint8)]
    for _ in range(d):
        zp.append(gmul(zp[-1], z))
    num = np.zeros(cand, np.uint8)  # omega(z), omega = S lambda mod x^d
    for i in range(d):
        om_i = np.bitwise_xor.reduce(np.stack([gmul(lam[:, j], s[:, i - j]) for j in range(i + 1)]), axis=0)
        num ^= gmul(om_i, zp[i])
    cut = np.bitwise_xor.reduce(np.stack([gmul(lam[:, i - k], zp[i]) for i in range(k, d)]), axis=0)  # x^k lambda(x) mod x^d at z
    ok = cut != 0
    assert (num != 0).all()
    e = np.where(ok, gmul(num, ginv(np.where(ok, cut, 1))), 0)
    s = s.copy()
    s[:, k] ^= e
    assert ok.sum() >= n
    return _finish(label, rng, s[ok][:n], expect=d, roots=roots[ok][:n])


def _leading_zeros(label, z, n=128):
    rng = Rng(label, n * 200)
    s = rng.take(n, NSYN).copy()
    s[:, :z] = 0
    s[:, z] = np.where(s[:, z] == 0, 1, s[:, z])
    return _finish(label, rng, s)


def _over(w, n=N_DEFAULT):
    label = "over_%d" % w
    rng = Rng(label, n * 1200)
    msg = rng.take(n, 110)
    words = np.concatenate([msg, reffix.rs_parity(msg)], axis=-1)
    pos = rng.distinct(n, 0, 119, w)
    val = rng.nonzero(n, w)
    for j in range(w):
        words[np.arange(n), pos[:, j]] ^= val[:, j]
    return Klass(label, words)


def _random(n=N_RANDOM):
    return Klass("random", Rng("random", n * 120).take(n, 120).copy())


def _filler(label, n, errors):
    rng = Rng(label, n * 400)
    msg = rng.take(n, 110)
    words = np.concatenate([msg, reffix.rs_parity(msg)], axis=-1)
    if errors:
        words[np.arange(n), rng.take(n).astype(np.int64) % 120] ^= rng.nonzero(n)
    return Klass(label, words, expect=errors, want=np.concatenate([msg, reffix.rs_parity(msg)], axis=-1))


@functools.lru_cache(maxsize=None)
def classes():
    """label -> Klass, in a fixed order"""
    out = {}

    def add(k):
        out[k.label] = k
    for d in range(1, 6):
        add(_root_class("real_%d" % d, d, 0))
    for d in range(1, 6):
        for m in range(1, d + 1):
            add(_root_class("pad_%d_%d" % (d, m), d, m))
    add(_deg2_noroot())
    add(_deg2_double())
    add(_deg2_r0())
    for d in (3, 4, 5):
        add(_nosplit(d))
    for k in range(2, 10):
        add(_short(k))
    add(_zero_s(0))
    add(_zero_s(1))
    for d in (1, 2, 3):
        add(_num1_zero(d))
    add(_deg6_ok())
    add(_leading_zeros("deg6_bad", 5))
    for z in range(6, 10):
        add(_leading_zeros("deg%d" % (z + 1), z))
    for w in range(6, 11):
        add(_over(w))
    add(_random())
    return out


VALUE_CLASSES = tuple(["real_%d" % d for d in range(1, 6)] + ["pad_%d_%d" % (d, m) for d in range(1, 6) for m in range(1, d + 1)]
                      + ["deg2_noroot", "deg2_double", "deg2_r0", "nosplit_3", "nosplit_4", "nosplit_5", "short_2", "short_3", "num1_zero_1", "num1_zero_2", "num1_zero_3", "deg6_ok"])


@functools.lru_cache(maxsize=None)
def fillers():
    return {"clean": _filler("clean", 512, 0), "single": _filler("single", 512, 1)}


# ---- tables of superframes -----------------------------------------------------------------------------------------------
class Pool:
    """all columns of all classes and the fillers in one array; take(label) cycles through a class's columns"""

    def __init__(self):
        ks = list(classes().values()) + list(fillers().values())
        self.words = np.concatenate([k.words for k in ks])
        self.labels = [k.label for k in ks]
        self.size = {k.label: len(k) for k in ks}
        self.off, o = {}, 0
        for k in ks:
            self.off[k.label] = o
            o += len(k)
        self.cnt = dict.fromkeys(self.labels, 0)
        self.label_of = np.repeat(np.arange(len(ks)), [len(k) for k in ks])

    def take(self, label):
        i = self.off[label] + self.cnt[label] % self.size[label]
        self.cnt[label] += 1
        return i


def superframes(pool, idx):
    """idx (nsf, rsdims) of pool columns -> p (nsf, 120 * rsdims): byte k of column j at k * rsdims + j"""
    nsf, r = idx.shape
    return np.ascontiguousarray(pool.words[idx].transpose(0, 2, 1)).reshape(nsf, 120 * r)


class Table:
    """name, rsdims, idx (nsf, rsdims) of pool columns, p, and `marks`: (context, class label, sf, column) of every
    special column, from which the tests count what was reached"""

    def __init__(self, name, pool, idx, marks):
        self.name, self.rsdims, self.idx, self.marks = name, idx.shape[1], idx, marks
        self.p = superframes(pool, idx)
        self.nsf = idx.shape[0]


def per_column_table(pool=None, limit=None):
    """RSDims 1: every column of every class a superframe of its own (limit: the first `limit` of each class)"""
    pool = pool or Pool()
    idx, marks = [], []
    for label, k in classes().items():
        n = len(k) if limit is None else min(limit, len(k))
        for i in range(n):
            marks.append(("column", label, len(idx), 0))
            idx.append(pool.off[label] + i)
    return Table("per_column" if limit is None else "per_column_%d" % limit, pool, np.array(idx)[:, None], marks)


COMPANY_LANES = (0, 31, 63)


def company_contexts():
    """(name, base filler, heavy classes, h, extra class or None)"""
    ctx = [("clean", "clean", (), 0, None), ("single", "single", (), 0, None)]
    heavy = [("d3_h%d" % h, ("real_3",), h) for h in (1, 12, 13, 63)] + [("d45_h%d" % h, ("real_4", "real_5"), h) for h in (1, 28, 29, 63)]
    for extra in (None, "deg6_bad", "deg6_ok"):
        for name, hv, h in heavy:
            ctx.append((name + ("+" + extra if extra else ""), "clean", hv, min(h, 62) if extra else h, extra))
    ctx.append(("all_deg6_ok", "deg6_ok", (), 0, None))
    return ctx


def company_table(pool=None, labels=None):
    """RSDims 1, one wave (64 consecutive superframes of a 256-superframe pass) per (context, class, lane): the special
    column at that lane, the other 63 as the context says"""
    pool = pool or Pool()
    rows, marks = [], []
    for name, base, hv, h, extra in company_contexts():
        for label in (labels or classes().keys()):
            for lane in COMPANY_LANES:
                wave = [pool.take(base) for _ in range(64)]
                others = [l for l in range(64) if l != lane]
                others = [others[(i * 37) % 63] for i in range(63)]  # 37 and 63 are coprime: a fixed spread
                for i in range(h):
                    wave[others[i]] = pool.take(hv[i % len(hv)])
                if extra:
                    wave[others[h]] = pool.take(extra)
                wave[lane] = pool.take(label)
                marks.append((name, label, 64 * len(rows) + lane, 0))
                rows.append(wave)
    return Table("company", pool, np.array(rows).reshape(-1, 1), marks)


FAIL_CLASSES = ("deg2_noroot", "nosplit_3", "deg6_bad")
ACCEPTED = ("pad_1_1", "deg6_ok", "short_2", "pad_3_2", "pad_5_5", "pad_2_1", "pad_4_4", "pad_5_3")
FIRST_FAILURE_DIMS = (2, 3, 24, 48, 64, 100, 256)
WIDE_DIMS = (257, 300, 512)
EXPORT_DIMS = (1, 24, 256, 257, 300)


def _fill(pool, r, sf):
    """a superframe of clean and single-error columns"""
    return [pool.take("single" if (j + sf) % 3 == 0 else "clean") for j in range(r)]


def _place(pool, row, marks, sf, ctx, cols):
    acc = 0
    for j in cols:
        if 0 <= j < len(row):
            label = ACCEPTED[(sf + acc) % len(ACCEPTED)]
            row[j] = pool.take(label)
            marks.append((ctx, label, sf, j))
            acc += 1


def first_failure_table(rsdims, pool=None):
    """superframes whose first failing column is of each class of FAIL_CLASSES at a spread of positions pf, with accepted
    special columns before it (written, summed) and after it (never output); every fourth superframe has no failure.
    The superframe count is odd, and no multiple of 256 // rsdims where that is above 1: the last group is partial."""
    pool = pool or Pool()
    r = rsdims
    pfs = sorted(set([0, 1, r // 3, r // 2, r - 2, r - 1] + list(range(0, r, max(1, r // 12)))) & set(range(r)))
    spb = max(1, 256 // r)
    specs = [(fc, pf, None) for fc in FAIL_CLASSES for pf in pfs]
    # superframes that straddle two wavefronts (local slot s of a pass holds lanes s*r .. s*r + r - 1): the failure in the
    # last column of the first wavefront and in the first column of the next one, in each such slot
    slots = [s for s in range(spb) if (s * r) // 64 != (s * r + r - 1) // 64] if r < 256 and 64 % r else []
    for side in (0, 1):
        for fc in FAIL_CLASSES:
            for s in slots:
                specs.append((fc, ((s * r) // 64 + 1) * 64 - s * r - 1 + side, s))
    rows, marks = [], []

    def accepted_only():
        sf = len(rows)
        row = _fill(pool, r, sf)
        _place(pool, row, marks, sf, "no_failure", [0, r // 2, r - 1])
        rows.append(row)
    for fc, pf, slot in specs:
        while slot is not None and len(rows) % spb != slot:
            accepted_only()
        sf = len(rows)
        row = _fill(pool, r, sf)
        _place(pool, row, marks, sf, "before_" + fc, [0, pf // 2, pf - 1][:pf])
        after = sorted({pf + 1, (pf + r) // 2, r - 1} - {pf})
        _place(pool, row, marks, sf, "after_" + fc, after)
        row[pf] = pool.take(fc)
        marks.append(("first_failure", fc, sf, pf))
        if pf + 2 < r and sf % 2 and pf + 2 not in after:  # a second failure of another form behind the first one
            row[pf + 2] = pool.take(FAIL_CLASSES[(FAIL_CLASSES.index(fc) + 1) % 3])
        rows.append(row)
        if len(rows) % 4 == 3:
            accepted_only()
    spb = max(1, 256 // r)
    while len(rows) % 2 == 0 or (spb > 1 and len(rows) % spb == 0):
        rows.append(_fill(pool, r, len(rows)))
    return Table("first_failure_%d" % r, pool, np.array(rows), marks)


def wide_table(rsdims, pool=None):
    """rsdims > 256: special columns in the first, a middle and the last 256-column chunk; a failure in the second chunk
    with accepted special columns before and after it; a failure in the first chunk (the later chunks are never read)"""
    pool = pool or Pool()
    r = rsdims
    second = min(r - 1, 270 if r < 512 else 300)
    rows, marks = [], []
    for k, fc in enumerate(FAIL_CLASSES + (None,)):
        for pf in ((second, 40, r - 1) if fc else (None,)):
            sf = len(rows)
            row = _fill(pool, r, sf)
            spots = sorted({5, 255, 256, r // 2, r - 2, r - 1, second - 3, second + 3} & set(range(r)) - {pf})
            if pf is None:
                _place(pool, row, marks, sf, "no_failure", spots)
            else:
                _place(pool, row, marks, sf, "before_" + fc, [j for j in spots if j < pf])
                _place(pool, row, marks, sf, "after_" + fc, [j for j in spots if j > pf])
                row[pf] = pool.take(fc)
                marks.append(("first_failure", fc, sf, pf))
            rows.append(row)
    for label in ("pad_5_5", "deg6_ok", "short_2", "short_6", "random"):  # whole chunks of one class
        sf = len(rows)
        row = [pool.take(label if 200 <= j < 290 else "clean") for j in range(r)]
        marks.extend(("chunk_of", label, sf, j) for j in range(200, min(290, r)))
        rows.append(row)
    return Table("wide_%d" % r, pool, np.array(rows), marks)


def export_table(rsdims, pool=None):
    """one superframe per class: the class's column in the middle (RSDims 1: alone), an accepted one before and after"""
    pool = pool or Pool()
    r = rsdims
    rows, marks = [], []
    for label in classes():
        sf = len(rows)
        row = _fill(pool, r, sf)
        if r > 2:
            _place(pool, row, marks, sf, "export_company", [1, r - 1])
        row[r // 2] = pool.take(label)
        marks.append(("export", label, sf, r // 2))
        rows.append(row)
    return Table("export_%d" % r, pool, np.array(rows), marks)


def pinned_tables():
    """the tables whose reference results are committed (tests/golden/reference_rs_paths.npy), in the file's order"""
    pool = Pool()
    tabs = [per_column_table(pool, limit=64)]
    tabs += [first_failure_table(r, pool) for r in FIRST_FAILURE_DIMS]
    tabs += [wide_table(r, pool) for r in WIDE_DIMS]
    tabs += [export_table(r, pool) for r in EXPORT_DIMS]
    return tabs


# ---- results: classification, non-vacuity, the pinned rows -----------------------------------------------------------------
def decode_columns(decode_word, words):
    """decode_word(word) -> (ret, patched word): every column -> (ret (n,) int32, patched (n, 120) uint8)"""
    ret = np.empty(words.shape[0], np.int32)
    fix = np.empty_like(words)
    for i, w in enumerate(words):
        ret[i], fix[i] = decode_word(w)
    return ret, fix


def non_vacuity(ret_of):
    """ret_of: label -> return values of a trusted decoder (the oracle, the reference build) for classes()[label].words.
    Asserts the conditions under which the classes test what they are meant to; by construction the reference meets them
    exactly.  -> counts for the log"""
    C = classes()
    assert set(ret_of) == set(C)
    for label, k in C.items():
        assert len(k) >= 64, label
        assert ret_of[label].shape == (len(k),)
    for label in VALUE_CLASSES:
        bad = np.flatnonzero(ret_of[label] != C[label].expect)
        assert bad.size == 0, "%s: columns %s do not return %d" % (label, bad[:8], C[label].expect)
    k6 = C["deg6_ok"]
    padroots = (k6.roots <= PAD).sum(axis=1)
    assert len(k6) >= 128 and (padroots == 0).sum() >= 32 and (padroots > 0).sum() >= 32, np.bincount(padroots)
    short = np.concatenate([ret_of["short_%d" % k] for k in (4, 5, 6)])
    assert (short >= 0).sum() >= 8 and (short == 6).sum() >= 2, np.unique(short, return_counts=True)
    rnd = ret_of["random"]
    assert (rnd >= 0).sum() >= 100, (rnd >= 0).sum()
    allret = np.concatenate(list(ret_of.values()))
    return {"columns": int(allret.size), "random_accepted": int((rnd >= 0).sum()), "short_4_6_accepted": int((short >= 0).sum()),
            "short_4_6_six_roots": int((short == 6).sum()), "deg6_ok_no_padding_root": int((padroots == 0).sum()),
            "deg6_ok_padding_root": int((padroots > 0).sum()), "accepted_degree_6": int((allret == 6).sum()),
            "accepted_degree_7_and_above": int((allret >= 7).sum())}


def pinned_rows(check_batch, tabs=None):
    """check_batch(p, rsdims, out_init) -> (ret, out): one row (rsdims, return value, FNV-1a-64 of the sentinel-initialised
    output, FNV-1a-64 of the input) per superframe of the pinned tables, as in reference_rs.npy"""
    rows = []
    for t in (tabs or pinned_tables()):
        ret, out = check_batch(t.p, t.rsdims, np.full((t.nsf, 110 * t.rsdims), reffix.RS_SENTINEL, np.uint8))
        rows.append(np.stack([np.full(t.nsf, t.rsdims, np.uint64), ret.astype(np.int64).view(np.uint64),
                              reffix.fnv1a64_rows(list(out)), reffix.fnv1a64_rows(list(t.p))], axis=1))
    return np.concatenate(rows)


def class_digests():
    """label -> FNV-1a-64 of the class's columns, row by row, folded: pins the generator itself"""
    return {label: "%016x" % reffix.fnv1a64(reffix.fnv1a64_rows(list(k.words)).view(np.uint8)) for label, k in classes().items()}


# ---- coverage: what the tables reach, counted from a trusted decoder's classification of their own columns ---------------
def pool_returns(pool, ret_of):
    """ret_of: label -> return values per class (a trusted decoder's) -> return value of every pool column"""
    F = fillers()
    return np.concatenate([ret_of[l] if l in ret_of else np.full(pool.size[l], F[l].expect, np.int32) for l in pool.labels])


def table_cells(pool, tabs, pool_ret):
    """(table, context, class) -> number of marked columns that are what the context says: a "first_failure" column must
    fail, a "before_" / "after_" / "no_failure" / "export_company" column must be accepted with at least one root, and
    nothing in front of a "first_failure" column may fail.  First-failure tables also count, for superframes that
    straddle wavefronts, whether the failure sits in the superframe's first wavefront or a later one."""
    cells = {}

    def count(key, n=1):
        cells[key] = cells.get(key, 0) + n
    for t in tabs:
        r = t.rsdims
        spb = max(1, 256 // r)
        colret = pool_ret[t.idx]  # (nsf, rsdims)
        for ctx, label, sf, col in t.marks:
            v = colret[sf, col]
            if ctx == "first_failure":
                ok = v == -1 and (colret[sf, :col] >= 0).all()
                if ok and r <= 256:
                    first, lane = ((sf % spb) * r) // 64, ((sf % spb) * r + col) // 64
                    if ((sf % spb) * r + r - 1) // 64 != first:
                        count((t.name, "straddle_first_wave" if lane == first else "straddle_later_wave", label))
                if ok and r > 256:
                    count((t.name, "failure_in_chunk_%d" % (col // 256), label))
            elif ctx.startswith(("before_", "after_", "no_failure", "export_company")):
                ok = v > 0
                if ok and r > 256:
                    count((t.name, ctx.split("_")[0] + "_chunk_%s" % ("first" if col < 256 else "last" if col // 256 == (r - 1) // 256 else "middle"), "*"))
            else:
                ok = True
            if ok:
                count((t.name, ctx, label))
                count((t.name, ctx, "*"))
    return cells


def assert_cells(cells):
    """every class x context cell the tests are meant to reach is reached"""
    def need(*key):
        assert cells.get(key, 0) > 0, "not reached: %s" % (key,)
    names = {k[0] for k in cells}
    if "company" in names:
        for ctx in company_contexts():
            for label in classes():
                need("company", ctx[0], label)
    for r in FIRST_FAILURE_DIMS:
        t = "first_failure_%d" % r
        if t not in names:
            continue
        for fc in FAIL_CLASSES:
            need(t, "first_failure", fc)
            need(t, "before_" + fc, "*")
            need(t, "after_" + fc, "*")
            if r >= 24:
                for label in ("pad_1_1", "deg6_ok", "short_2"):
                    assert cells.get((t, "before_" + fc, label), 0) + cells.get((t, "after_" + fc, label), 0) > 0, (t, fc, label)
            if r in (3, 24, 100):
                need(t, "straddle_first_wave", fc)
                need(t, "straddle_later_wave", fc)
        need(t, "no_failure", "*")
    for r in WIDE_DIMS:
        t = "wide_%d" % r
        if t not in names:
            continue
        for fc in FAIL_CLASSES:
            need(t, "failure_in_chunk_1", fc)
            need(t, "failure_in_chunk_0", fc)
            need(t, "before_" + fc, "*")
            need(t, "after_" + fc, "*")
        need(t, "before_chunk_first", "*")
        need(t, "after_chunk_last", "*")
        need(t, "no_chunk_first", "*")
        need(t, "no_chunk_last", "*")
        for label in ("pad_5_5", "deg6_ok", "short_2", "short_6", "random"):
            need(t, "chunk_of", label)
    for r in EXPORT_DIMS:
        t = "export_%d" % r
        if t not in names:
            continue
        for label in classes():
            need(t, "export", label)
