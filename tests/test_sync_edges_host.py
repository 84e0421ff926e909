"""CPU-only: inputs directed at the edges of vit_ofdm_sync_dev's arithmetic and geometry ("From the coarse start",
include/viterbi_amd.h), and the proof on the numpy model of tests/test_sync_host.py that every input has the property it
is aimed at.  tests/test_gpu_sync_edges.py runs the same inputs through the kernel.
  1  planted guard correlations: gamma is an exact small sum that lands on every branch of the arctangent, on its
     boundaries, in the denormal range and on the ties of the rint
  2  an amplitude ladder from 2^12 down to 2^-39 (the metric becomes denormal) and the frame the 2^12 bound is about
  3  partial zeros, equal paths and thresholds: the first-maximum and first-over-threshold rules one at a time
  4  the guard loop's geometry: Gw = G - 2W against the workgroup's size TPB = max(64, nfft/8)
  5  frames outside the domain between good ones
There are no tolerances: what is asserted is asserted exactly."""
import numpy as np
import pytest

from test_fft_host import F32, nco_model, twiddles_model
from test_sync_host import ATAN_C, Params, nacc_of, prs_table, std_bins, sync_model, transmit_frames, turn_model

NCO_BITS = 12
TINY = float(2.0 ** -126)  # the smallest normal binary32
_cache = {}


class Case:
    """one call's inputs: samples, parameters, the reference symbol, the coarse table; what the builder knows besides"""

    def __init__(self, x, prm, prs, coarse, **meta):
        self.x, self.prm, self.prs, self.coarse = x, prm, prs, np.asarray(coarse, np.int64)
        self.nframes = len(self.coarse)
        self.__dict__.update(meta)

    def with_params(self, **kw):
        p = self.prm
        args = dict(cp_symbols=p.cp_symbols, thr=p.thr, backoff=p.backoff)
        args.update(kw)
        meta = {k: v for k, v in self.__dict__.items() if k not in ("x", "prm", "prs", "coarse", "nframes")}
        return Case(self.x, Params(p.nfft, p.guard, p.nsyms, p.W, p.M, **args), self.prs, self.coarse, **meta)


def cached(fn):
    def wrapper(*args):
        key = (fn.__name__,) + args
        if key not in _cache:
            _cache[key] = fn(*args)
        return _cache[key]
    wrapper.__name__ = fn.__name__
    return wrapper


class Result:
    def __init__(self, start, rot, info, turn, detail):
        self.start, self.rot, self.info, self.turn, self.detail = start, rot, info, turn, detail
        self.mhat, self.tau = info[:, 0].view(np.int32), info[:, 1].view(np.int32)
        f = info[:, 2:].view(F32)
        self.g_re, self.g_im, self.E, self.metric, self.pmax, self.psum = (f[:, i] for i in range(6))
        self.floats = f


def model_of(case, skip=()):
    """the model's outputs for a case, with the model's own tables; frames in `skip` are not computed"""
    coarse = case.coarse.copy()
    coarse[list(skip)] = -1
    detail = []
    out = sync_model(case.x, coarse, case.prm, case.prs, twiddles_model(case.prm.nfft), nco_model(NCO_BITS), NCO_BITS,
                     detail=detail)
    by_frame = {d["t"]: d for d in detail}
    return Result(*out, [by_frame.get(t) for t in range(case.nframes)])


def rint_half_even(v):
    """rint of a binary64 value, in Python's own arithmetic"""
    return round(float(v))  # Python rounds halves to even


def step_of(turn, nfft):
    """(-rint(turn * 2^32/nfft)) mod 2^32; the product is exact in binary64 too"""
    return (-rint_half_even(float(turn) * (2.0 ** 32 / nfft))) % (1 << 32)


def frames(shape, nframes, seed, m=None, eps=None, delta=None, snr_db=15.0, echo=None, bins=None, scale=None):
    """transmitted frames with silence between them; frame t has the offset m[t] + eps[t] carrier spacings and the
    coarse start true[t] + delta[t], odd for odd t and even for even t -> (x, true, coarse, prs)"""
    nfft, G, nsyms, W, M = shape
    prm = Params(nfft, G, nsyms, W, M)
    rng = np.random.default_rng(seed)
    bins = std_bins(nfft) if bins is None else np.asarray(bins)
    prs = prs_table(rng, nfft, bins)
    m = rng.integers(-max(M - 1, 0), max(M - 1, 0) + 1, nframes) if m is None else np.asarray(m)
    eps = rng.uniform(-0.4, 0.4, nframes) if eps is None else np.asarray(eps)
    delta = rng.integers(-W, W + 1, nframes) if delta is None else np.asarray(delta)
    lead, tail, pos = [], [2 * W + 2] * nframes, 0
    for t in range(nframes):
        lead.append(2 * W + 2 + (t - (pos + 2 * W + 2 + G + int(delta[t]))) % 2)
        pos += lead[t] + nsyms * (nfft + G) + tail[t]
    x, true, _ = transmit_frames(rng, prm, prs, bins, nframes, m + eps, lead=lead, tail=tail, echo=echo, snr_db=snr_db,
                                 scale=scale)
    coarse = true + delta
    assert [int(c) % 2 for c in coarse] == [t % 2 for t in range(nframes)]
    return x, true, coarse, prs


def repeat_frame(x, coarse0, n):
    """n copies of one frame's buffer, placed so that the coarse starts are even and odd in turn -> (x, coarse starts, the
    copies' offsets)"""
    chunks, offs, pos = [], [], 0
    for t in range(n):
        gap = (t - pos - int(coarse0)) % 2
        chunks += [np.zeros(gap, np.complex64), x]
        offs.append(pos + gap)
        pos += gap + x.size
    offs = np.array(offs, np.int64)
    assert [int(c) % 2 for c in offs + int(coarse0)] == [t % 2 for t in range(n)]
    return np.concatenate(chunks), offs + int(coarse0), offs


# ---- 1: planted guard correlations ----------------------------------------------------------------------------------

PLANT_NFFT = (64, 256, 2048, 8192)
# G - 2W exceeds NACC everywhere, so that two elements can share an accumulator
PLANT_SHAPES = {64: (64, 80, 3, 4, 3), 256: (256, 200, 3, 10, 4), 2048: (2048, 504, 3, 100, 4), 8192: (8192, 1200, 2, 64, 2)}
OCTANTS = [(3.0, 1.25), (1.25, 3.0), (-1.25, 3.0), (-3.0, 1.25), (-3.0, -1.25), (-1.25, -3.0), (1.25, -3.0), (3.0, -1.25)]
DIAGONALS = [(1.0, 1.0), (-1.0, 1.0), (-1.0, -1.0), (1.0, -1.0)]
AXES = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)]


def turn_at_the_diagonal():
    """the polynomial at q = 1 by Horner's rule, one binary32 operation at a time: what the graph gives for ay == ax,
    where no reflection is taken"""
    p = ATAN_C[6]
    for c in ATAN_C[5::-1]:
        p = F32(F32(p * F32(1)) + c)
    return F32(p * F32(1))


@cached
def tie_gammas(nfft):
    """gammas (1, q) with turn * 2^32/nfft = j + 1/2 exactly, j = 0 ... 3: found among the binary32 neighbours of
    q = 2 pi (j + 1/2) nfft / 2^32 with the model's arctangent -> [(j, q)]"""
    found = []
    for j in range(4):
        q0 = np.array(2 * np.pi * (j + 0.5) * nfft / 2.0 ** 32, F32)
        cand = (int(q0.view(np.uint32)) + np.arange(-4000, 4001)).astype(np.uint32).view(F32)
        v = turn_model(np.ones_like(cand), cand).astype(np.float64) * (2.0 ** 32 / nfft)
        hits = cand[v == j + 0.5]
        assert hits.size, "no tie at %d + 1/2 near q = %r" % (j, float(q0))
        found.append((j, float(hits[0])))
    return found


@cached
def planted_gammas(nfft):
    """-> [(name, [(k, a, b), ...], (gamma.re, gamma.im))]: pairs (x[n], x[n + nfft]) = (a, b) at element k of symbol 1's
    guard range, everything else of the range 0"""
    G, W = PLANT_SHAPES[nfft][1], PLANT_SHAPES[nfft][3]
    Gw, nacc = G - 2 * W, nacc_of(nfft)
    lo = max(0, Gw - nfft)  # an element below it has its b inside the range
    one = (1.0, 0.0)
    singles = [("octant %d" % i, g) for i, g in enumerate(OCTANTS)]
    singles += [("diagonal %d" % i, g) for i, g in enumerate(DIAGONALS)]
    singles += [("axis %d" % i, g) for i, g in enumerate(AXES)]
    singles += [("minus one, minus zero", (-1.0, -0.0)), ("just under the negative real axis", (-1.0, -2.0 ** -30)),
                ("denormal imaginary part", (2.0 ** -100, 2.0 ** -140)), ("denormal q", (2.0 ** 12, 2.0 ** -130)),
                ("q of four denormal units", (2.0 ** 12, -2.0 ** -135)), ("q underflows", (-2.0 ** 12, 2.0 ** -149)),
                ("components 2^40 apart", (2.0 ** 20, 2.0 ** -20)), ("components 2^40 apart, steep", (-2.0 ** -20, -2.0 ** 20))]
    for j, q in tie_gammas(nfft):
        singles += [("tie at %d + 1/2" % j, (1.0, q)), ("tie at -(%d + 1/2)" % j, (1.0, -q))]
    out = [("nothing planted", [], (0.0, 0.0))]
    for t, (name, g) in enumerate(singles):
        k = lo + (7 * t + 5) % (min(Gw, nacc) - lo)  # another accumulator, lane and wavefront every time
        out.append((name, [(k, one, g)], g))
    # two elements of one accumulator: k and k + NACC.  At nfft 64 NACC = nfft, so the first pair's b is the second's a
    k = 3
    out.append(("one accumulator twice", [(k, one, one), (k + nacc, one, (0.5, -3.0))], (1.5, -3.0)))
    # accumulators 2 and NACC/2 + 2 meet in the last addition of the tree
    out.append(("the last level of the tree", [(lo + 2, one, (3.0, 1.0)), (nacc // 2 + 2, one, (-1.0, 2.0))], (2.0, 3.0)))
    for name, pairs, g in out:
        ks = {k for k, _, _ in pairs}
        assert all(k < Gw and (k + nfft >= Gw or k + nfft in ks) for k in ks), name
    return out


@cached
def planted_case(nfft):
    shape = PLANT_SHAPES[nfft]
    _, G, nsyms, W, M = shape
    x1, true, coarse, prs = frames(shape, 1, 3000 + nfft, m=[1], eps=[0.3], delta=[-2])
    plan = planted_gammas(nfft)
    x, coarse, offs = repeat_frame(x1, coarse[0], len(plan))
    for c, (name, pairs, _) in zip(coarse, plan):
        n0 = int(c) + nfft + W  # c + S - G + W
        assert n0 > int(c) - W + nfft - 1  # behind the reference window
        x[n0:n0 + G - 2 * W] = 0
        written = {}
        for k, a, b in pairs:
            for n, v in ((n0 + k, a), (n0 + k + nfft, b)):
                v = np.complex64(complex(*v))
                assert written.setdefault(n, v) == v, name
                x[n] = v
    return Case(x, Params(nfft, G, nsyms, W, M, cp_symbols=1, thr=0.5, backoff=1), prs, coarse, plan=plan, offs=offs,
                true=true[0] + offs)


@cached
def planted_model(nfft):
    return model_of(planted_case(nfft))


@pytest.mark.parametrize("nfft", PLANT_NFFT)
def test_planted_gammas_are_exact(nfft):
    """the model's gamma words are the planted sums; steps B to D still see the real symbol"""
    case, r = planted_case(nfft), planted_model(nfft)
    want = np.array([g for _, _, g in case.plan], F32) + F32(0)  # accumulators start at +0: no -0 comes out
    assert np.array_equal(want.astype(np.float64), np.array([g for _, _, g in case.plan]))  # representable
    assert np.array_equal(r.g_re.view(np.uint32), want[:, 0].view(np.uint32))
    assert np.array_equal(r.g_im.view(np.uint32), want[:, 1].view(np.uint32))
    assert (r.pmax > 0).all() and (r.psum > 0).all() and (r.metric > 0).all()
    assert len(case.plan) >= 35


@pytest.mark.parametrize("nfft", PLANT_NFFT)
def test_planted_turns_take_every_branch(nfft):
    """the turn of every planted gamma: exact on the axes, the diagonals and the boundaries, the denormal results kept,
    within the header's 2^-23 turn of binary64 atan2 everywhere, and rot = the rint of it, ties to even"""
    case, r = planted_case(nfft), planted_model(nfft)
    turn = dict(zip([name for name, _, _ in case.plan], r.turn))
    d = turn_at_the_diagonal()
    assert 0.25 - float(d) != float(d)  # so a reflection taken at ay == ax would show
    for i, want in enumerate([d, F32(0.5) - d, -(F32(0.5) - d), -d]):
        assert turn["diagonal %d" % i].view(np.uint32) == F32(want).view(np.uint32)
    assert [float(turn["axis %d" % i]) for i in range(4)] == [0.0, 0.25, 0.5, -0.25]
    assert turn["minus one, minus zero"] == 0.5 and turn["just under the negative real axis"] == -0.5
    assert turn["nothing planted"] == 0 and turn["q underflows"] == 0.5
    c0 = float(ATAN_C[0])
    assert turn["denormal q"] == F32(c0 * 2.0 ** -142) and 0 < turn["denormal q"] < TINY
    assert turn["q of four denormal units"] == -F32(2.0 ** -149) == -F32(c0 * 2.0 ** -147)  # 0.64 units round to one
    assert turn["denormal imaginary part"] == F32(c0 * 2.0 ** -40)  # q = 2^-40: the polynomial rounds to C0
    for i in range(8):  # the open octants, in order
        assert i / 8 < float(turn["octant %d" % i]) % 1.0 < (i + 1) / 8
    g = np.array([g for _, _, g in case.plan])
    ref = np.arctan2(g[:, 1], g[:, 0]) / (2 * np.pi)
    err = np.abs(r.turn.astype(np.float64) - ref)
    assert np.minimum(err, 1 - err).max() < 2.0 ** -23
    # the step: rint with ties to even, in Python's arithmetic
    spacing = (1 << 32) // nfft
    for t in range(case.nframes):
        assert int(r.rot[t, 1]) == (step_of(r.turn[t], nfft) - int(r.mhat[t]) * spacing) % (1 << 32), case.plan[t][0]
        assert r.detail[t]["step_frac"] == step_of(r.turn[t], nfft)
    for name in ("axis 2", "minus one, minus zero"):  # half a turn per symbol: the step times nfft is 2^31
        assert (step_of(turn[name], nfft) * nfft) % (1 << 32) == 1 << 31
    assert step_of(turn["just under the negative real axis"], nfft) == (1 << 31) // nfft


@pytest.mark.parametrize("nfft", PLANT_NFFT)
def test_planted_ties_of_the_rint(nfft):
    """at least four frames have turn * 2^32/nfft at an integer + 1/2 exactly: both signs, even and odd integer parts"""
    case, r = planted_case(nfft), planted_model(nfft)
    v = r.turn.astype(np.float64) * (2.0 ** 32 / nfft)
    ties = v[np.abs(v) % 1.0 == 0.5]
    assert ties.size >= 8
    assert {(bool(t > 0), int(abs(t)) % 2) for t in ties} == {(True, 0), (True, 1), (False, 0), (False, 1)}
    assert {0.5, -0.5, 1.5, -1.5, 2.5, -2.5} <= set(ties.tolist())
    # ties to even: 1/2 -> 0, 3/2 -> 2, 5/2 -> 2
    steps = {float(t): (-int(s["step_frac"])) % (1 << 32) for t, s in zip(v, r.detail) if abs(t) % 1.0 == 0.5}
    assert steps[0.5] == 0 and steps[-0.5] == 0 and steps[1.5] == 2 and steps[-1.5] == (1 << 32) - 2 and steps[2.5] == 2


# ---- 2: the amplitude ladder ------------------------------------------------------------------------------------------

LADDER_SHAPES = {64: (64, 16, 4, 4, 3), 256: (256, 63, 4, 15, 8), 2048: (2048, 504, 3, 100, 16)}
LOW_RUNGS = [-36, -38, -39]
RUNGS = {64: list(range(12, -35, -2)) + LOW_RUNGS, 256: list(range(12, -35, -2)) + LOW_RUNGS,
         2048: [12, 8, 2, -4, -10, -16, -22, -28, -32, -34] + LOW_RUNGS}


@cached
def ladder_case(nfft):
    """one noisy frame with an integer and a fractional offset and a timing error, its largest sample magnitude scaled to
    2^r by an exact power of two for every rung r; components under 2^-40 are 0.  The floor is applied to the real and
    the imaginary part of a sample, not to its magnitude: stricter than the header's wording, so every sample is inside
    the domain whichever way that is read, but the low rungs lose more than a floor on the magnitude would take and are
    not the upper rungs scaled (the metric falls by 2^-7 from 2^-38 to 2^-39 at nfft 64, where scaling alone gives 2^-4)."""
    shape = LADDER_SHAPES[nfft]
    _, G, nsyms, W, M = shape
    x1, true, coarse, prs = frames(shape, 1, 4000 + nfft, m=[-2], eps=[0.3], delta=[-(W // 2)], scale=1.0)
    top = np.abs(x1.astype(np.complex128)).max()
    base = (x1.astype(np.complex128) / top * (1 - 2.0 ** -20)).astype(np.complex64)
    assert 1 - 2.0 ** -19 < np.abs(base.astype(np.complex128)).max() <= 1.0
    x, coarse, offs = repeat_frame(base, coarse[0], len(RUNGS[nfft]))
    for part in (x.real, x.imag):
        for r, o in zip(RUNGS[nfft], offs):
            part[o:o + base.size] *= F32(2.0 ** r)
        part[np.abs(part) < 2.0 ** -40] = 0
    return Case(x, Params(nfft, G, nsyms, W, M, thr=0.5), prs, coarse, rungs=RUNGS[nfft], offs=offs, true=true[0] + offs,
                frame_len=base.size)


@cached
def ladder_model(nfft):
    return model_of(ladder_case(nfft))


def in_domain(x):
    """every component 0 or of magnitude 2^-40 or more, every sample's magnitude 2^12 at most"""
    comp = np.abs(np.concatenate([x.real, x.imag]))
    return bool(((comp == 0) | (comp >= 2.0 ** -40)).all()) and bool(np.abs(x.astype(np.complex128)).max() <= 2.0 ** 12)


@pytest.mark.parametrize("nfft", sorted(LADDER_SHAPES))
def test_ladder(nfft):
    """inside the domain on every rung; m^, tau and the start the same on every rung down to 2^-34; every info float
    finite; the metric of m^ a nonzero denormal on a rung at nfft 64 and 256 (the model: 0x1.b998p-135 and 0x1.94ae2p-128
    at 2^-38; below 2^-34 the zeroed components change the frame, see ladder_case).  At nfft 2048 the model reaches no
    denormal metric inside the domain: the smallest it reaches is 0x1.668788p-126 on the lowest rung, 2^-39, in the last
    binade of the normal range.  That word is asserted, and that it is the smallest of the ladder."""
    case, r = ladder_case(nfft), ladder_model(nfft)
    assert in_domain(case.x)
    for rung, o in zip(case.rungs, case.offs):
        top = np.abs(case.x[o:o + case.frame_len].astype(np.complex128)).max()
        assert 2.0 ** (rung - 1) < top <= 2.0 ** rung  # 2^rung before the small components went to 0
    high = np.array(case.rungs) >= -34
    assert high.sum() == len(case.rungs) - 3 and case.rungs[0] == 12
    assert (r.mhat[high] == -2).all() and (r.tau[high] == r.tau[0]).all()
    assert np.array_equal(r.start[high], case.true[high])
    assert np.isfinite(r.floats).all()
    print("nfft %d: metric[m^] per rung %s" % (nfft, ["2^%d: %s" % (a, float(b).hex()) for a, b in zip(case.rungs, r.metric)]))
    denormal = (r.metric > 0) & (r.metric < TINY)
    if nfft == 2048:
        assert not denormal.any() and r.metric.argmin() == len(case.rungs) - 1
        assert TINY <= r.metric[-1] < 2 * TINY and r.metric[-1] == F32(float.fromhex("0x1.668788p-126"))
    else:
        assert denormal.any()
    others = np.delete(r.floats, 3, axis=1)
    assert ((others == 0) | (np.abs(others) >= TINY)).all()  # every other info float stays normal


LARGEST_SHAPES = {64: (64, 16, 3, 4, 3), 8192: (8192, 600, 2, 64, 4)}


@cached
def largest_case(nfft):
    """two adjacent carriers of amplitude 2^11 in every sample of the buffer: sample magnitudes reach 2^12 exactly, the
    input the header's overflow bound is about"""
    shape = LARGEST_SHAPES[nfft]
    _, G, nsyms, W, M = shape
    prm = Params(nfft, G, nsyms, W, M)
    bins = std_bins(nfft)
    prs = prs_table(np.random.default_rng(4100 + nfft), nfft, bins)
    k0 = 5
    assert prs[k0] != 0 and prs[k0 + 1] != 0
    coarse = np.array([W + 3, W + 3 + prm.span() + 4], np.int64)
    n = np.arange(int(coarse[-1]) - W + prm.span())
    x = (2.0 ** 11 * (np.exp(2j * np.pi * k0 * n / nfft) + np.exp(2j * np.pi * (k0 + 1) * n / nfft))).astype(np.complex64)
    for part in (x.real, x.imag):
        part[np.abs(part) < 2.0 ** -40] = 0  # where a sine should have been 0
    return Case(x, prm, prs, coarse)


@pytest.mark.parametrize("nfft", sorted(LARGEST_SHAPES))
def test_largest_result(nfft):
    """the model stays finite; the metric is 2^44 nfft^4 to within a factor of two - 2^96 at nfft 8192, the largest
    word any frame inside the domain produces"""
    case = largest_case(nfft)
    r = model_of(case)
    assert in_domain(case.x) and np.abs(case.x.astype(np.complex128)).max() == 2.0 ** 12
    assert np.isfinite(r.floats).all()  # (every shift meets the one large D with an R of magnitude 1: m^ is any of them)
    assert (r.metric > 2.0 ** 43 * float(nfft) ** 4).all() and (r.metric < 2.0 ** 45 * float(nfft) ** 4).all()


# ---- 3: partial zeros and the threshold -------------------------------------------------------------------------------

ZERO_SHAPE = (256, 63, 4, 15, 8)


@cached
def partial_zero_case():
    """frame 0: the reference window all zero, the guards real; frame 1: the guards (both halves of every pair) all zero,
    the window real, no fractional offset; frames 2, 3: untouched.  Noise-free, cp_symbols 1."""
    nfft, G, nsyms, W, M = ZERO_SHAPE
    x, true, coarse, prs = frames(ZERO_SHAPE, 4, 5000, m=[1, 2, -3, 0], eps=[0.3, 0.0, -0.2, 0.1], delta=[2, 3, -W, W],
                                  snr_db=None)
    c = int(coarse[0])
    x[c - W:c - W + nfft] = 0
    n0 = int(coarse[1]) + nfft + W
    x[n0:n0 + G - 2 * W] = 0
    x[n0 + nfft:n0 + nfft + G - 2 * W] = 0
    return Case(x, Params(nfft, G, nsyms, W, M, cp_symbols=1, thr=0.5, backoff=2), prs, coarse, true=true)


def test_window_zero_and_guards_zero():
    case = partial_zero_case()
    nfft, G, nsyms, W, M = ZERO_SHAPE
    r = model_of(case)
    # the window zero: every metric and every power ties at 0, the first of each wins; the guards still give a turn
    assert r.mhat[0] == -M and r.tau[0] == 0 and r.psum[0] == 0 and r.pmax[0] == 0 and r.metric[0] == 0
    assert r.turn[0] != 0 and r.E[0] > 0
    assert not r.detail[0]["metric"].any() and not r.detail[0]["p"].any()
    assert int(r.rot[0, 1]) == (step_of(r.turn[0], nfft) + M * ((1 << 32) // nfft)) % (1 << 32)
    assert r.start[0] == case.coarse[0] - W - 2
    # the guards zero: no turn, no step; the window still gives the integer offset and the start
    assert r.turn[1] == 0 and r.g_re[1] == 0 and r.g_im[1] == 0 and r.E[1] == 0
    assert r.mhat[1] == 2 and r.tau[1] == W - 3 and r.start[1] + 2 == case.true[1]
    assert int(r.rot[1, 1]) == (-2 * ((1 << 32) // nfft)) % (1 << 32)
    assert np.array_equal(r.start[2:] + 2, case.true[2:]) and r.mhat[2:].tolist() == [-3, 0]
    assert r.tau[2:].tolist() == [2 * W, 0]


WRAP_SHAPE = (64, 16, 3, 4, 3)


@cached
def wrapped_prs_case():
    """a reference symbol that is zero on bins 0 ... M only: R[k] is zero for k = 0 ... M + 1 and the sums reach the
    wrapped indices k - 1 = nfft - 1 and (k + m) mod nfft with signal on both sides; offsets -M, +M, 0"""
    nfft, G, nsyms, W, M = WRAP_SHAPE
    x, true, coarse, prs = frames(WRAP_SHAPE, 3, 5100, m=[-M, M, 0], eps=[0.2, -0.2, 0.1], delta=[1, -2, 3], snr_db=None,
                                  bins=np.arange(M + 1, nfft))
    assert not prs[:M + 1].any() and (prs[M + 1:] != 0).all()
    return Case(x, Params(nfft, G, nsyms, W, M, thr=0.5), prs, coarse, true=true)


def test_wrapped_reference_bins():
    case = wrapped_prs_case()
    r = model_of(case)
    M = WRAP_SHAPE[4]
    assert r.mhat.tolist() == [-M, M, 0] and np.array_equal(r.start, case.true)
    for d in r.detail:  # a single maximum each: no tie decides these
        assert (d["metric"] == d["metric"].max()).sum() == 1


@cached
def edge_path_case():
    """thr 1: the strongest path at n = 0, at n = 2W, and at n = 2W with a path twice as strong at 2W + 1, outside the
    search (pmax and tau must not see it)"""
    nfft, G, nsyms, W, M = ZERO_SHAPE
    x, true, coarse, prs = frames(ZERO_SHAPE, 3, 5200, m=[1, -1, 2], eps=[0.2, -0.3, 0.1], delta=[W, -W, -W], snr_db=None,
                                  echo=[(0.0, 1), (0.0, 1), (2.0, 1)])
    return Case(x, Params(nfft, G, nsyms, W, M, thr=1.0), prs, coarse, true=true)


def test_strongest_path_at_the_ends_of_the_search():
    case = edge_path_case()
    W = ZERO_SHAPE[3]
    r = model_of(case)
    assert r.tau.tolist() == [0, 2 * W, 2 * W] and np.array_equal(r.start, case.true)
    for t, n in enumerate([0, 2 * W, 2 * W]):
        p = r.detail[t]["p"]
        assert p[n] == r.pmax[t] == p[:2 * W + 1].max() and (p[:2 * W + 1] == p[n]).sum() == 1
    p = r.detail[2]["p"]
    assert p[2 * W + 1] > 2 * r.pmax[2] and p.argmax() == 2 * W + 1


PAIR_SHAPE = (64, 50, 3, 20, 0)


@cached
def equal_paths_case():
    """a reference symbol on even bins only (the spectrum of an impulse pair nfft/2 apart): conj Z is zero on odd k, the
    last butterflies of its transform add and subtract zeros, and h[n] = h[n + nfft/2] bit for bit.  Frame 0 and the
    noisy frame 2 put the pair at n = 3 and 35, frame 1 at 8 and 40 = 2W.  thr 1, M 0 (R[k] is zero everywhere)."""
    nfft, G, nsyms, W, M = PAIR_SHAPE
    bins = [k for k in std_bins(nfft) if k % 2 == 0]
    x, true, coarse, prs = frames(PAIR_SHAPE, 2, 5300, m=[0, 0], eps=[0.0, 0.0], delta=[W - 3, W - 8], snr_db=None, bins=bins)
    xn, truen, coarsen, prsn = frames(PAIR_SHAPE, 1, 5300, m=[0], eps=[0.0], delta=[W - 3], snr_db=15.0, bins=bins)
    assert np.array_equal(prs, prsn)
    return Case(np.concatenate([x, xn]), Params(nfft, G, nsyms, W, M, thr=1.0), prs, np.append(coarse, coarsen + x.size),
                true=np.append(true, truen + x.size))


def test_equal_paths_take_the_first():
    case = equal_paths_case()
    nfft, _, _, W, _ = PAIR_SHAPE
    r = model_of(case)
    for t, n in enumerate([3, 8, 3]):
        p = r.detail[t]["p"]
        assert p[n].view(np.uint32) == p[n + nfft // 2].view(np.uint32) and n + nfft // 2 <= 2 * W
        assert np.array_equal(p[:nfft // 2], p[nfft // 2:])
        assert p[n] == r.pmax[t] > 0 and r.tau[t] == n  # the smaller index
        assert (p[:2 * W + 1] == r.pmax[t]).sum() == 2
    assert np.array_equal(r.start, case.true) and not r.metric.any()


THR_TINY = float(2.0 ** -149)  # the smallest positive denormal
THR_LOW = float(2.0 ** -24)
THR_DEEP = float(2.0 ** -72)


@cached
def threshold_case(nfft, thr):
    return ladder_case(nfft).with_params(thr=thr)


@pytest.mark.parametrize("nfft", [64, 256])
def test_thresholds_in_the_denormal_range(nfft):
    """thr = 2^-149: thr * pmax rounds to 0 wherever pmax <= 1/2, every power reaches it and tau is 0; on the high rungs
    the level is a nonzero denormal.  thr = 2^-24 on the ladder: p[n] is the square of a sum of samples, not a fourth
    power like the metric; the strongest path of a frame whose largest sample is 2^-39 has a power near 2^-65, so
    2^-24 * pmax stays normal on every rung (asserted).  thr = 2^-72 is what makes the level itself a nonzero denormal
    on the low rungs, and both are run."""
    r = model_of(threshold_case(nfft, THR_TINY))
    level = F32(THR_TINY) * r.pmax
    assert (level == 0).sum() >= 3 and ((level > 0) & (level < TINY)).sum() >= 3
    assert (r.tau[level == 0] == 0).all()
    r = model_of(threshold_case(nfft, THR_LOW))
    assert (F32(THR_LOW) * r.pmax >= TINY).all()
    r = model_of(threshold_case(nfft, THR_DEEP))
    level = F32(THR_DEEP) * r.pmax
    assert ((level > 0) & (level < TINY)).sum() >= 2 and (level >= TINY).sum() >= 2


# ---- 4: the guard loop's geometry -------------------------------------------------------------------------------------
# (shape, frames, cp_symbols of each call, what it is aimed at)
GEOMETRY = [
    ((512, 126, 4, 31, 5), 4, [1, 2, 3], "Gw == TPB"),
    ((1024, 252, 4, 62, 12), 3, [1, 3], "Gw == TPB"),
    ((64, 16, 41, 4, 3), 3, list(range(1, 41)), "Gw divides TPB"),
    ((128, 3, 40, 1, 5), 4, [1, 2, 39], "Gw == 1"),
    ((128, 3, 515, 1, 5), 3, [255, 256, 257, 511, 512, 513], "totals"),
    ((128, 5, 172, 1, 5), 3, [85, 86, 170, 171], "totals"),
    ((1024, 3, 514, 1, 4), 3, [511, 512, 513], "totals"),
    ((256, 300, 3, 10, 8), 4, [1, 2], "Gw > 4 TPB"),
]


@cached
def geometry_case(i):
    shape, nframes, cps, _ = GEOMETRY[i]
    nfft, G, nsyms, W, M = shape
    x, true, coarse, prs = frames(shape, nframes, 6000 + i)
    return Case(x, Params(nfft, G, nsyms, W, M), prs, coarse, true=true, cps=cps)


def test_geometry_shapes_are_what_they_are_aimed_at():
    """TPB = max(64, nfft/8); the loop steps by dq = TPB / Gw, dr = TPB % Gw, four elements per thread and pass.  Totals
    cp_symbols * Gw of 4 TPB r - 1, 4 TPB r and 4 TPB r + 1, r = 1 and 2, are hit exactly with Gw = 1 at TPB 64 (and r = 1 at TPB 128);
    with Gw = 3 at TPB 64, 256 and 512 are no multiples of 3 and the nearest totals on each side are taken: 255 and 258,
    510 and 513."""
    totals = {}
    for shape, nframes, cps, aim in GEOMETRY:
        nfft, G, nsyms, W, M = shape
        tpb, Gw = nacc_of(nfft), G - 2 * W
        assert 3 <= nframes <= 4 and all(1 <= cp <= nsyms - 1 for cp in cps) and 2 * W < G
        if aim == "Gw == TPB":
            assert Gw == tpb and tpb % Gw == 0
        elif aim == "Gw divides TPB":
            assert 1 < Gw < tpb and tpb % Gw == 0 and cps == list(range(1, 41)) and nsyms == 41
        elif aim == "Gw == 1":
            assert Gw == 1
        elif aim == "Gw > 4 TPB":
            assert Gw > 4 * tpb
        else:
            totals.setdefault((tpb, Gw), set()).update(cp * Gw for cp in cps)
    assert totals[(64, 1)] == {256 * r + d for r in (1, 2) for d in (-1, 0, 1)}
    assert totals[(128, 1)] == {511, 512, 513}
    assert totals[(64, 3)] == {255, 258, 510, 513}


@pytest.mark.parametrize("i", [0, 2, 3, 5, 7])
def test_geometry_frames_on_the_model(i):
    """the builders give frames the model synchronises: odd and even coarse starts, every start found (15 dB)"""
    case = geometry_case(i)
    assert {int(c) % 2 for c in case.coarse} == {0, 1}
    r = model_of(case.with_params(cp_symbols=case.cps[-1]))
    assert np.array_equal(r.start, case.true)


# ---- 5: frames outside the domain -------------------------------------------------------------------------------------

BAD_SHAPE = (256, 63, 8, 15, 8)
BAD_FRAMES = {1: complex(np.nan, np.nan), 3: complex(np.inf, -np.inf), 5: complex(3e38, 3e38)}


@cached
def out_of_domain_case():
    """good, NaN, good, Inf, good, 3e38 (finite, overflows in the first product), good"""
    nfft, G, nsyms, W, M = BAD_SHAPE
    x, true, coarse, prs = frames(BAD_SHAPE, 7, 7000)
    for t, v in BAD_FRAMES.items():
        x[true[t] - G:true[t] - G + nsyms * (nfft + G)] = v
    return Case(x, Params(nfft, G, nsyms, W, M, thr=0.5, backoff=3), prs, coarse, true=true, bad=sorted(BAD_FRAMES))


def test_frames_outside_the_domain():
    case = out_of_domain_case()
    prm = case.prm
    for t, c in enumerate(case.coarse):
        seen = case.x[c - prm.W:c - prm.W + prm.span()]
        if t in case.bad:
            inside = seen[2 * prm.W + prm.guard:-2 * prm.W]  # without the silence the coarse error can reach into
            assert (~np.isfinite(inside)).all() or (np.abs(inside.real) == F32(3e38)).all()
        else:
            assert np.isfinite(seen).all()
    with np.errstate(over="ignore"):
        assert not np.isfinite(F32(3e38) * F32(3e38))
    r = model_of(case, skip=case.bad)
    good = [t for t in range(case.nframes) if t not in case.bad]
    assert np.array_equal(r.start[good] + 3, case.true[good]) and (r.start[case.bad] == -1).all()
