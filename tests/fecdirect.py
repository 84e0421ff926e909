"""Syndrome-directed RS(204,188) rows: test inputs that choose the path a row takes through the packet-mode FEC decoder
(tests/test_fec_paths_host.py, tests/test_gpu_fec_paths.py).

The syndrome map of the shortened code is onto: for any sixteen byte positions the 16x16 Vandermonde system over GF(2^8)
is invertible, so a codeword with sixteen bytes adjusted has ANY chosen syndrome vector (row_with_syndromes).  A test can
therefore pick what Berlekamp-Massey will find - final length, degree, root set, repeated or missing roots, roots among the
51 virtual padding positions - instead of waiting for "codeword plus random errors" to produce it.

Conventions (csrc/vit_packet.hip): byte k of a row is the coefficient of x^(203-k), its degree d = 203 - k;
S_i = sum_d c_d alpha^(i d), i = 0 ... 15; an error of value Y at degree d has X = alpha^d, S_i = Y X^i, and the locator
Lambda(x) = prod (1 + X x) vanishes at 1/X; d = 204 ... 254 are the padding of RS(255,239).

Two things are kept apart.  The CLASSIFIER (bm_trace, classify) is a plain full-length Berlekamp-Massey with 18
coefficients on Python ints: it proves that a row takes the path its label names, nothing else.  The REFERENCE for bytes
and nerr is always decode_row_model of tests/test_packet_host.py, which takes the Euclid route.

Pure numpy / Python: no GPU, no library."""
import collections
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from test_packet_host import (AL, COLS, FEC_DATA_BYTES, FEC_FRAME_BYTES, FEC_PACKETS, FEC_REC_DTYPE, FEC_SLOTS, IDX,  # noqa: E402
                              MULL, NCODE, NPAR, SLOT, TCORR, decode_row_model, encode_rows, fec_hdr, ginv, gsolve,
                              miscorrection_row, padding_root_row, pdeg, peval, pmul, syndromes)

NBM = NPAR + 2  # coefficients the classifier keeps


# ---- builders -------------------------------------------------------------------------------------------------------------
def apow(e):
    return AL[e % 255]


def power_sums(degs, vals):
    """S_i = sum_j vals[j] alpha^(i degs[j]), i = 0 ... 15; degs 0 ... 254"""
    S = [0] * NPAR
    for d, v in zip(degs, vals):
        for i in range(NPAR):
            S[i] ^= MULL[v][apow(i * d)]
    return S


def random_codeword(rng):
    return encode_rows(rng.integers(0, 256, COLS, dtype=np.uint8))


def random_degs(rng, n, exclude=(), hi=NCODE):
    """n distinct degrees below hi, none of them in `exclude`"""
    pool = [d for d in range(hi) if d not in set(exclude)]
    return [pool[int(k)] for k in rng.permutation(len(pool))[:n]]


def row_with_syndromes(rng, S, degs=None):
    """a random codeword with the 16 bytes at the distinct degrees `degs` (< 204) adjusted so that its syndrome vector is
    exactly S"""
    degs = random_degs(rng, NPAR) if degs is None else list(degs)
    assert len(degs) == NPAR and len(set(degs)) == NPAR and all(0 <= d < NCODE for d in degs)
    e = gsolve([[apow(i * d) for d in degs] for i in range(NPAR)], [int(s) for s in S])
    assert e is not None
    row = random_codeword(rng)
    for d, v in zip(degs, e):
        row[NCODE - 1 - d] ^= v
    assert [int(x) for x in syndromes(row)] == [int(s) for s in S]
    return row


def row_with_errors(rng, degs, vals):
    """(received, sent): a random codeword with the non-zero values `vals` added at the distinct degrees `degs` (< 204)"""
    assert len(degs) == len(vals) and len(set(degs)) == len(degs) and all(0 <= d < NCODE for d in degs) and all(vals)
    cw = random_codeword(rng)
    row = cw.copy()
    for d, v in zip(degs, vals):
        row[NCODE - 1 - d] ^= v
    return row, cw


def constrained_values(degs, zero_syn, first):
    """values of n = len(degs) errors (degrees 0 ... 254) that make the syndromes S_i, i in zero_syn, vanish: the leading
    n - len(zero_syn) values are `first` (an int or a list), the others follow from the zero_syn equations.  None if
    that system is singular or a value comes out zero."""
    first = [first] if isinstance(first, int) else list(first)
    n, z = len(degs), len(zero_syn)
    assert len(first) == n - z and z < n and all(first)
    if z == 0:
        return first
    A = [[apow(i * d) for d in degs[n - z:]] for i in zero_syn]
    y = [0] * z
    for r, i in enumerate(zero_syn):
        for d, v in zip(degs, first):
            y[r] ^= MULL[v][apow(i * d)]
    rest = gsolve(A, y)
    if rest is None or not all(rest):
        return None
    return first + rest


def locator(degs):
    """prod (1 + alpha^d x), lowest coefficient first"""
    lam = [1]
    for d in degs:
        lam = pmul(lam, [1, apow(d)])
    return lam


def recurrence(lam, init):
    """the sixteen words with S_0 ... S_(L-1) = init and S_n = sum_j lam[j] S_(n-j) from n = L on, L = len(lam) - 1"""
    L = len(lam) - 1
    S = [int(x) for x in init]
    assert len(S) == L
    for n in range(L, NPAR):
        v = 0
        for j in range(1, L + 1):
            v ^= MULL[lam[j]][S[n - j]]
        S.append(v)
    return S[:NPAR]


def irreducible_quadratic(rng):
    """1 + a x + b x^2 without a root in the field"""
    while True:
        q = [1, int(rng.integers(1, 256)), int(rng.integers(1, 256))]
        if all(peval(q, x) for x in range(1, 256)):
            return q


# ---- the classifier ---------------------------------------------------------------------------------------------------------
def bm_trace(S):
    """full-length Berlekamp-Massey, 18 coefficients -> (L, deg Lambda, Lambda, steps); steps[r-1] = (dsc != 0, grew, dL)"""
    S = [int(s) for s in S]
    lam, b, L, steps = [1] + [0] * (NBM - 1), [1] + [0] * (NBM - 1), 0, []
    for r in range(1, NPAR + 1):
        dsc = 0
        for k in range(r):
            dsc ^= MULL[lam[k]][S[r - 1 - k]]
        grew = dsc != 0 and 2 * L <= r - 1
        t = [lam[0]] + [lam[k] ^ MULL[dsc][b[k - 1]] for k in range(1, NBM)]
        if grew:
            inv = ginv(dsc)
            b = [MULL[x][inv] for x in lam]
            dL = r - 2 * L
            L = r - L
        else:
            b = [0] + b[:-1]
            dL = 0
        lam = t
        steps.append((dsc != 0, grew, dL))
    return L, pdeg(lam), lam, steps


def bm_trace_cut(S):
    """the same recursion with Lambda and B cut at degree 8 exactly as vit_fec_kernel cuts them: terms above x^8 are
    never formed, the shift of B drops its x^8 term -> (L, deg, Lambda (9 coefficients), bad = L > 8 or deg != L)"""
    S = [int(s) for s in S]
    n = TCORR + 1
    lam, b, L = [1] + [0] * TCORR, [1] + [0] * TCORR, 0
    for r in range(1, NPAR + 1):
        dsc = 0
        for k in range(n):
            if k < r:
                dsc ^= MULL[lam[k]][S[r - 1 - k]]
        grew = dsc != 0 and 2 * L <= r - 1
        if grew:
            inv = ginv(dsc)
            nb = [MULL[x][inv] for x in lam]
        else:
            nb = [0] + b[:TCORR]
        if dsc:
            lam = [lam[0]] + [lam[k] ^ MULL[dsc][b[k - 1]] for k in range(1, n)]
        if grew:
            L = r - L
        b = nb
    deg = max(pdeg(lam), 0)
    return L, deg, lam, L > TCORR or deg != L


def roots_of(lam):
    """the degrees d = 0 ... 254 with Lambda(alpha^-d) = 0, and those of them where Lambda' vanishes too"""
    lam = lam[:pdeg(lam) + 1]
    der = [lam[j] if j % 2 else 0 for j in range(1, len(lam))] or [0]  # characteristic 2: only odd terms survive
    roots = [d for d in range(255) if peval(lam, apow(255 - d)) == 0]
    return roots, [d for d in roots if peval(der, apow(255 - d)) == 0]


def classify(row):
    """the labels of the paths a row takes, from bm_trace of its syndromes and from the roots of Lambda over all 255
    positions"""
    S = [int(x) for x in syndromes(np.asarray(row, np.uint8))]
    if not any(S):
        return {"clean"}
    out = set()
    lead = next(i for i, s in enumerate(S) if s)
    if lead:
        out |= {"S0=0", "lead%d" % lead}
    zeros = [i for i, s in enumerate(S) if s == 0]
    if len(zeros) == 1 and zeros[0] >= 1:
        out.add("lone_S%d=0" % zeros[0])
    L, deg, lam, steps = bm_trace(S)
    out.add("L%d" % L)
    if L > TCORR:
        out.add("L>8")
    if deg < L:
        out.add("deg<L")
    grown = [r for r, st in enumerate(steps) if st[1]]
    nonzero = [r for r, st in enumerate(steps) if st[0]]
    if any(not steps[r][0] for r in range(grown[0] + 1, nonzero[-1])):
        out.add("zero_dsc_mid")
    Lb = 0
    for nz, grew, dL in steps:
        if grew and dL >= 2 and Lb >= 1:
            out |= {"jump>=2", "jump_to_%d" % (Lb + dL)}
        Lb += dL
    if L <= TCORR and deg == L:
        for j in range(1, L):
            if lam[j] == 0:
                out.add("lam%d=0@L%d" % (j, L))
        roots, multiple = roots_of(lam)
        pad = [d for d in roots if d >= NCODE]
        out.add("roots%d" % len(roots))
        out |= {"root@%d" % d for d in roots}
        if multiple:
            out.add("repeated_root")
        if len(roots) < L:
            out.add("few_roots")
        else:
            out.add("pad_roots%d" % len(pad))
    return out


# ---- the directed set -----------------------------------------------------------------------------------------------------
# group: the family (placement tests take one representative of each); name: the cell of the issue's list;
# nerr / want: what construction says decode_row_model returns; need: the classifier's labels the row must carry
Entry = collections.namedtuple("Entry", "group name row nerr want need")

SEAMS = (0, 63, 64, 127, 128, 191, 192, 203)
DRAW_CAP = 6000


def _errors_entry(rng, group, name, degs, vals, need):
    row, cw = row_with_errors(rng, degs, vals)
    return Entry(group, name, row, len(degs), cw, set(need) | {"L%d" % len(degs), "pad_roots0"} | {"root@%d" % d for d in degs})


def _fail_entry(rng, group, name, S, need):
    row = row_with_syndromes(rng, S)
    return Entry(group, name, row, -1, row.copy(), set(need))


def _nz(rng, n):
    return [int(x) for x in rng.integers(1, 256, n)]


def _correctable(rng, out):
    # S_0 = 0, n = 2 ... 8
    for n in range(2, 9):
        degs = random_degs(rng, n)
        out.append(_errors_entry(rng, "s0_zero", "s0_zero_n%d" % n, degs, constrained_values(degs, [0], _nz(rng, n - 1)), {"lead1"}))
    # m leading zero syndromes with m + 1 and with 8 errors
    for m in range(1, 8):
        for n, tag in ((m + 1, "min"), (8, "n8")):
            degs = random_degs(rng, n)
            vals = constrained_values(degs, list(range(m)), _nz(rng, n - m))
            out.append(_errors_entry(rng, "lead", "lead%d_%s" % (m, tag), degs, vals, {"S0=0", "lead%d" % m}))
    # a lone zero syndrome
    for k in range(1, NPAR):
        for _ in range(DRAW_CAP):
            n = int(rng.integers(2, 9))
            degs = random_degs(rng, n)
            vals = constrained_values(degs, [k], _nz(rng, n - 1))
            if vals is not None and [i for i, s in enumerate(power_sums(degs, vals)) if s == 0] == [k]:
                break
        else:
            raise AssertionError("lone_S%d=0: draw cap" % k)
        out.append(_errors_entry(rng, "lone", "lone_s%d" % k, degs, vals, {"lone_S%d=0" % k}))
    # a zero discrepancy between the first growth and the last non-zero discrepancy: seeded rejection sampling
    jump, flat = [], []
    for _ in range(DRAW_CAP):
        n = int(rng.integers(3, 9))
        degs, vals = random_degs(rng, n), _nz(rng, n)
        L, deg, lam, steps = bm_trace(power_sums(degs, vals))
        grown = [r for r, st in enumerate(steps) if st[1]]
        nonzero = [r for r, st in enumerate(steps) if st[0]]
        if not any(not steps[r][0] for r in range(grown[0] + 1, nonzero[-1])):
            continue
        Lb, jumped = 0, False
        for nz, grew, dL in steps:
            jumped |= grew and dL >= 2 and Lb >= 1
            Lb += dL
        if jumped and len(jump) < 4:
            jump.append((degs, vals))
        elif not jumped and len(flat) < 6:
            flat.append((degs, vals))
        if len(jump) >= 2 and len(jump) + len(flat) >= 8:
            break
    else:
        raise AssertionError("zero_dsc_mid: draw cap")
    for k, (degs, vals) in enumerate(jump):
        out.append(_errors_entry(rng, "zero_dsc", "zero_dsc_jump_%d" % k, degs, vals, {"zero_dsc_mid", "jump>=2"}))
    for k, (degs, vals) in enumerate(flat):
        out.append(_errors_entry(rng, "zero_dsc", "zero_dsc_flat_%d" % k, degs, vals, {"zero_dsc_mid"}))
    # an interior coefficient of the locator zero: L - 1 free positions, the last from lambda_j = e_j + X e_(j-1) = 0
    for j, L in [(1, L) for L in range(3, 9)] + [(j, 8) for j in range(2, 8)] + [(j, j + 1) for j in range(2, 7)]:
        for _ in range(DRAW_CAP):
            degs = random_degs(rng, L - 1)
            e = locator(degs)
            if e[j] == 0 or e[j - 1] == 0:
                continue
            x = MULL[e[j]][ginv(e[j - 1])]
            d = next(k for k in range(255) if AL[k] == x)
            if d < NCODE and d not in degs:
                break
        else:
            raise AssertionError("lam%d=0@L%d: draw cap" % (j, L))
        out.append(_errors_entry(rng, "lam_zero", "lam%d_zero_L%d" % (j, L), degs + [d], _nz(rng, L), {"lam%d=0@L%d" % (j, L)}))
    # every position with every value: row i has its error at d = i mod 204 with value i + 1
    for i in range(255):
        out.append(_errors_entry(rng, "single", "single", [i % NCODE], [i + 1], ()))
    # eight errors with a root on each lane and quarter seam of the search, and one row with all of them
    for d in SEAMS:
        degs = [d] + random_degs(rng, 7, exclude=[d])
        out.append(_errors_entry(rng, "seam", "seam_%d" % d, degs, _nz(rng, 8), ()))
    out.append(_errors_entry(rng, "seam", "seam_all", list(SEAMS), _nz(rng, 8), ()))


def _uncorrectable(rng, out):
    # final L = 9 ... 16: m = 8 ... 15 leading zeros, the rest random
    for m in range(8, NPAR):
        S = [0] * m + _nz(rng, 1) + [int(x) for x in rng.integers(0, 256, NPAR - m - 1)]
        out.append(_fail_entry(rng, "L>8", "final_L%d" % (m + 1), S, {"L%d" % (m + 1), "L>8", "lead%d" % m}))
    # a late jump: the power sums of n errors with S_k altered, k >= 8 + n: L goes from n to k + 1 - n > 8
    for n in range(1, 5):
        for k in sorted({8 + n, NPAR - 1}):
            S = power_sums(random_degs(rng, n), _nz(rng, n))
            S[k] ^= int(rng.integers(1, 256))
            out.append(_fail_entry(rng, "late_jump", "late_jump_n%d_k%d" % (n, k), S,
                                   {"L%d" % (k + 1 - n), "L>8", "jump>=2", "jump_to_%d" % (k + 1 - n)}))
    # L <= 8 with deg Lambda < L: S = (s, 0, ..., 0), and a free first word in front of the power sums of L - 1 errors
    out.append(_fail_entry(rng, "deg<L", "deg_lt_L1", _nz(rng, 1) + [0] * (NPAR - 1), {"L1", "deg<L"}))
    for L in range(2, 9):
        for _ in range(DRAW_CAP):
            S = (_nz(rng, 1) + power_sums(random_degs(rng, L - 1), _nz(rng, L - 1)))[:NPAR]
            Lt, deg, lam, steps = bm_trace(S)
            if Lt == L and deg == L - 1:
                break
        else:
            raise AssertionError("deg_lt_L%d: draw cap" % L)
        out.append(_fail_entry(rng, "deg<L", "deg_lt_L%d" % L, S, {"L%d" % L, "deg<L"}))
    # deg = L <= 8 but fewer than L roots in the field: an irreducible quadratic factor; a repeated root
    for L in (2, 5, 8):
        for _ in range(DRAW_CAP):
            lam = pmul(irreducible_quadratic(rng), locator(random_degs(rng, L - 2)))
            S = recurrence(lam, _nz(rng, L))
            t = bm_trace(S)
            if t[0] == L and t[2][:L + 1] == lam:
                break
        else:
            raise AssertionError("irreducible_L%d: draw cap" % L)
        out.append(_fail_entry(rng, "irreducible", "irreducible_L%d" % L, S, {"L%d" % L, "few_roots", "roots%d" % (L - 2)}))
    for L in (2, 4, 8):
        for _ in range(DRAW_CAP):
            degs = random_degs(rng, L - 1)
            lam = pmul(locator(degs), [1, apow(degs[0])])
            S = recurrence(lam, _nz(rng, L))
            t = bm_trace(S)
            if t[0] == L and t[2][:L + 1] == lam:
                break
        else:
            raise AssertionError("repeated_L%d: draw cap" % L)
        out.append(_fail_entry(rng, "repeated", "repeated_L%d" % L, S,
                               {"L%d" % L, "few_roots", "repeated_root", "roots%d" % (L - 1), "root@%d" % degs[0]}))
    # L distinct roots, k of them in the padding d = 204 ... 254
    for L in (2, 8):
        degs = random_degs(rng, L - 1) + [NCODE + random_degs(rng, 1, hi=255 - NCODE)[0]]
        out.append(_fail_entry(rng, "pad_k1", "pad_k1_L%d" % L, power_sums(degs, _nz(rng, L)),
                               {"L%d" % L, "pad_roots1"} | {"root@%d" % d for d in degs}))
    for L in (1, 8):
        degs = [NCODE + d for d in random_degs(rng, L, hi=255 - NCODE)]
        out.append(_fail_entry(rng, "pad_all", "pad_all_L%d" % L, power_sums(degs, _nz(rng, L)),
                               {"L%d" % L, "pad_roots%d" % L} | {"root@%d" % d for d in degs}))
    # a root at exactly d = 204 beside the same row with that root at d = 203, which is correctable
    others, vals = random_degs(rng, 2, exclude=[NCODE - 1]), _nz(rng, 3)
    out.append(_errors_entry(rng, "pad_204", "root_203", [NCODE - 1] + others, vals, ()))
    out.append(_fail_entry(rng, "pad_204", "root_204", power_sums([NCODE] + others, vals),
                           {"L3", "pad_roots1", "root@204"} | {"root@%d" % d for d in others}))
    for L in (1, 4):
        degs = [254] + random_degs(rng, L - 1)
        out.append(_fail_entry(rng, "pad_254", "root_254_L%d" % L, power_sums(degs, _nz(rng, L)),
                               {"L%d" % L, "pad_roots1", "root@254"}))
    # the two directed rows the packet tests already have
    for _ in range(3):
        row, want = miscorrection_row(rng)
        out.append(Entry("miscorrection", "miscorrection", row, 8, want, {"L8", "pad_roots0"}))
        row = padding_root_row(rng)
        out.append(Entry("padding_root", "padding_root", row, -1, row.copy(), {"L8", "pad_roots1"}))


def expected_counts():
    """name -> how many rows of the directed set carry it"""
    c = collections.Counter()
    c.update("s0_zero_n%d" % n for n in range(2, 9))
    c.update("lead%d_%s" % (m, tag) for m in range(1, 8) for tag in ("min", "n8"))
    c.update("lone_s%d" % k for k in range(1, NPAR))
    c.update("lam1_zero_L%d" % L for L in range(3, 9))
    c.update("lam%d_zero_L8" % j for j in range(2, 8))
    c.update("lam%d_zero_L%d" % (j, j + 1) for j in range(2, 7))
    c["single"] = 255
    c.update("seam_%d" % d for d in SEAMS)
    c["seam_all"] = 1
    c.update("final_L%d" % L for L in range(9, 17))
    c.update("late_jump_n%d_k%d" % (n, k) for n in range(1, 5) for k in sorted({8 + n, NPAR - 1}))
    c.update("deg_lt_L%d" % L for L in range(1, 9))
    c.update("irreducible_L%d" % L for L in (2, 5, 8))
    c.update("repeated_L%d" % L for L in (2, 4, 8))
    c.update(["pad_k1_L2", "pad_k1_L8", "pad_all_L1", "pad_all_L8", "root_203", "root_204", "root_254_L1", "root_254_L4"])
    c["miscorrection"] = 3
    c["padding_root"] = 3
    return c


GROUPS = ("s0_zero", "lead", "lone", "zero_dsc", "lam_zero", "single", "seam", "L>8", "late_jump", "deg<L", "irreducible",
          "repeated", "pad_k1", "pad_all", "pad_204", "pad_254", "miscorrection", "padding_root")


@functools.lru_cache(maxsize=None)
def directed_set():
    """the whole set, seeded and deterministic, in a fixed order; the counts of expected_counts() are asserted here"""
    rng = np.random.default_rng(204188)
    out = []
    _correctable(rng, out)
    _uncorrectable(rng, out)
    have = collections.Counter(e.name for e in out)
    zd = {k: v for k, v in have.items() if k.startswith("zero_dsc_")}
    njump = sum(v for k, v in zd.items() if k.startswith("zero_dsc_jump_"))
    assert sum(zd.values()) >= 8 and njump >= 1, zd
    rest = collections.Counter({k: v for k, v in have.items() if k not in zd})
    assert rest == expected_counts(), (rest - expected_counts(), expected_counts() - rest)
    assert {e.group for e in out} == set(GROUPS)
    for e in out:
        e.row.setflags(write=False)
        e.want.setflags(write=False)
    return tuple(out)


def representatives():
    """group -> one entry; correctable and uncorrectable groups both occur"""
    reps = {}
    prefer = {"lead": "lead7_n8", "lam_zero": "lam1_zero_L8", "seam": "seam_all", "L>8": "final_L9", "pad_204": "root_204",
              "deg<L": "deg_lt_L8", "irreducible": "irreducible_L8", "repeated": "repeated_L8", "pad_k1": "pad_k1_L8",
              "pad_all": "pad_all_L8", "s0_zero": "s0_zero_n8", "late_jump": "late_jump_n4_k12"}
    for e in directed_set():
        if e.group not in reps and prefer.get(e.group, e.name) == e.name:
            reps[e.group] = e
    assert set(reps) == set(GROUPS)
    return reps


# ---- frames and their model -----------------------------------------------------------------------------------------------
def frames_of_rows(rows):
    """rows (F, 12, 204) -> F FEC frames (F, 2472): the rows through the interleaver, the nine FEC headers, padding 0"""
    rows = np.asarray(rows, np.uint8)
    frames = np.zeros((rows.shape[0], FEC_FRAME_BYTES), np.uint8)
    frames[:, IDX] = rows
    for c in range(FEC_PACKETS):
        frames[:, FEC_DATA_BYTES + SLOT * c:FEC_DATA_BYTES + SLOT * c + 2] = fec_hdr(c)
    return frames


def clean_rows(rng, n):
    return encode_rows(rng.integers(0, 256, (n, COLS), dtype=np.uint8))


class RowModel:
    """decode_row_model, remembered per distinct row (clean rows are decided by their syndromes, in bulk)"""

    def __init__(self):
        self.memo = {}

    def row(self, row):
        key = row.tobytes()
        if key not in self.memo:
            self.memo[key] = decode_row_model(row)
        return self.memo[key]

    def frames(self, frames):
        """frames (F, 2472) -> (decoded (F, 2472), records (F,)): fec_frame_model of every frame"""
        frames = np.array(frames, np.uint8).reshape(-1, FEC_FRAME_BYTES)
        rec = np.zeros(frames.shape[0], FEC_REC_DTYPE)
        rows = frames[:, IDX]
        dirty = syndromes(rows).any(axis=-1)
        for f, r in zip(*np.nonzero(dirty)):
            rows[f, r], rec["nerr"][f, r] = self.row(rows[f, r])
        frames[:, IDX] = rows
        for c in range(FEC_PACKETS):
            h = frames[:, FEC_DATA_BYTES + SLOT * c:FEC_DATA_BYTES + SLOT * c + 2]
            rec["hdr_ok"] |= ((h[:, 0] == fec_hdr(c)[0]) & (h[:, 1] == fec_hdr(c)[1])).astype(np.uint16) << np.uint16(c)
        rec["status"] = (rec["nerr"] < 0).any(axis=1)
        return frames, rec


def heavy_rows(rng, n):
    """n rows beyond the code's reach: 9 ... 20 random errors on a codeword, every fourth row plain random bytes"""
    rows = clean_rows(rng, n)
    for k in range(n):
        if k % 4 == 3:
            rows[k] = rng.integers(0, 256, NCODE, dtype=np.uint8)
        else:
            w = int(rng.integers(9, 21))
            pos = rng.permutation(NCODE)[:w]
            rows[k, pos] ^= rng.integers(1, 256, w, dtype=np.uint8)
    return rows


# ---- sync -----------------------------------------------------------------------------------------------------------------
def sync_model_fast(stream):
    """sync_model without its loops: a slot i that carries the header of FEC packet c counts for the one phase p with
    (i - p) mod 103 = 94 + c"""
    stream = np.asarray(stream, np.uint8)
    nslots = stream.size // SLOT
    h = stream[:nslots * SLOT].reshape(nslots, SLOT)
    score = np.zeros(FEC_SLOTS, np.int64)
    i = np.arange(nslots)
    for c in range(FEC_PACKETS):
        hit = (h[:, 0] == fec_hdr(c)[0]) & (h[:, 1] == fec_hdr(c)[1])
        score += np.bincount((i[hit] - (FEC_SLOTS - FEC_PACKETS) - c) % FEC_SLOTS, minlength=FEC_SLOTS)
    return score.astype(np.uint32)


def sync_stream(rng, nslots, phase, stray=6):
    """random slots with the nine FEC headers where `phase` puts them, and a few headers in the wrong place"""
    st = rng.integers(0, 256, SLOT * nslots, dtype=np.uint8)
    for i in range(nslots):
        m = (i - phase) % FEC_SLOTS
        if m >= FEC_SLOTS - FEC_PACKETS:
            st[SLOT * i:SLOT * i + 2] = fec_hdr(m - (FEC_SLOTS - FEC_PACKETS))
    for i in rng.integers(0, nslots, stray):
        st[SLOT * i:SLOT * i + 2] = fec_hdr(int(rng.integers(0, 12)))
    return st
