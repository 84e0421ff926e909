"""CPU-only: the inputs of tests/test_gpu_tii_edges.py - vit_ofdm_tii_dev at the caps and edges of its geometry - and the
conditions under which they mean something, checked with tii_model (tests/test_tii_host.py) alone.  The kernels' partition
sizes and the caps of the argument rules come from TII_GEOMETRY of the package:

  slots   Gp*C around one and four trips of the group kernel's 256 threads, up to the 1024 slots its LDS holds, Gp = 32
          with bit 31 of a mask set and clear, and at nfft 2048 a table that puts every bin into exactly one pair;
  navg    255 and 256 frames per estimate, skipped frames at both ends of a group, a ragged group of one;
  tiny    1, 3 and 15 slots, 8 repetitions;
  ties    slots that name the same pairs: equal energies at the median's rank and at the threshold;
  launch  a group's words do not depend on nframes, at 1024 slots.

Out of scope, and not forgotten: nothing in these kernels strides over the grid - a workgroup owns a frame or a group - so
there is no second trip of a launch to test; the grid-stride loops of the acquisition kernels are spoken of in
tests/test_acq_edges_host.py."""
import numpy as np
import pytest

from test_fft_host import F32, twiddles_model
from test_iqfmt_host import INT_FORMATS, quantise
from test_tii_host import Tii, decide_model, masks_of, random_pairs, rank_select, tii_model

IQ_F32 = 0
# (Gp, C): Gp*C = 255, 256, 257, 771, 1023, 1024, 1024, 1024 at the published sizes
SLOT_SHAPES = [(5, 51), (8, 32), (1, 257), (3, 257), (31, 33), (32, 32), (2, 512), (1, 1024)]
SLOT_NFFT = (2048, 4096)
NAVG_RUNS = [(255, 257), (255, 513), (256, 257), (256, 513)]  # (navg, nframes) at the published cap
NAVG_SHAPE = (64, 4, 3, 2)
TINY_SHAPES = [(1, 1, 8), (3, 1, 8), (3, 5, 2)]  # (Gp, C, R) at nfft 64
TIE_SHAPES = [(4, 4), (3, 5)]  # an even and an odd slot count
TIE_CLASS = (1, 6, 9, 13)      # the slots that name one pair
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def int_format(i):
    """one integer format per case, in rotation"""
    return INT_FORMATS[i % len(INT_FORMATS)]


def as_format(x, fmt):
    """-> (what the device gets and the model reads: complex64 (n,) or raw (n, 2), the model's fmt argument)"""
    if fmt == IQ_F32:
        return np.asarray(x, np.complex64), None
    raw, scale = quantise(x, fmt)
    return raw, (fmt, scale)


def slot_nrep(nfft, GC):
    """repetitions: at 2048 as many as fit, up to 4 - so 256 and 1024 slots fill the spectrum; at 4096 one pair fewer than
    fits, so that random_pairs can start at an odd bin"""
    return min(4, nfft // 2 // GC) if nfft == 2048 else min(4, (nfft // 2 - 1) // GC)


def pair_table(rng, nfft, Gp, C_, R):
    """random_pairs, or - where 2*R*Gp*C = nfft and its odd starting bin does not fit - every even bin as a lower bin, in
    random order: every bin of the spectrum in exactly one pair -> uint16 (R, Gp, C)"""
    if 2 * R * Gp * C_ < nfft:
        return random_pairs(rng, nfft, Gp, C_, R)
    assert 2 * R * Gp * C_ == nfft
    lower = 2 * rng.permutation(nfft // 2)
    assert sorted(np.concatenate([lower, lower + 1]).tolist()) == list(range(nfft))
    return lower.reshape(R, Gp, C_).astype(np.uint16)


def planted_slots(rng, Gp, C_):
    """the slots (b, c) that carry energy in every frame: the top group in comb 0 and not in the last comb, a comb in
    every trip of the comb loop, and a few anywhere; fewer than a quarter of all -> (set of on, one slot kept off)"""
    if C_ == 1:
        return ({(Gp // 2, 0)} if Gp > 1 else {(0, 0)}), ((0, 0) if Gp > 1 else None)
    on, off = {(Gp - 1, 0), (0, C_ - 1 if Gp > 1 else C_ - 2)}, (Gp - 1, C_ - 1)
    for c in range(257, C_ - 1, 256):
        on.add((int(rng.integers(0, Gp)), c))
    for _ in range(min(Gp * C_ // 8, 24)):
        on.add((int(rng.integers(0, Gp)), int(rng.integers(0, C_))))
    on.discard(off)
    return on, off


def windows(rng, nfft, pairs, nframes, on, noise=1.0, amp=(3.0, 6.0)):
    """Gaussian samples of power `noise`; in every frame's window the pairs of the slots `on` (a set, or one dict slot ->
    amplitude per frame) stand out of it.  The windows lie at odd and even positions 3 ... 40 samples apart ->
    (x complex128, starts int64, offset)"""
    R, Gp, C_ = pairs.shape
    offset = -(nfft + 13)
    w0 = np.cumsum((rng.integers(3, 41, nframes) | 1) + nfft) - nfft  # odd gaps: odd, even, odd, ...
    assert (w0 % 2 == 1).any() and (nframes < 2 or (w0 % 2 == 0).any())
    n = int(w0[-1]) + nfft + 5
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5 * noise)
    for t in range(nframes):
        Z = np.zeros(nfft, np.complex128)
        slots = on[t] if isinstance(on, list) else {s: rng.uniform(*amp) for s in sorted(on)}
        for (b, c), a in slots.items():
            k = pairs[:, b, c].astype(np.int64)
            Z[k] = a * np.sqrt(nfft) * np.exp(2j * np.pi * rng.random(R))
            Z[k + 1] = a * np.sqrt(nfft) * np.exp(2j * np.pi * rng.random(R))
        x[w0[t]:w0[t] + nfft] += np.fft.ifft(Z)
    return x, (w0 - offset).astype(np.int64), offset


def check_masks(words, Gp, on=(), off=None):
    """every group that counted a frame has the planted bits set, a bit set and a bit clear"""
    m = masks_of(words)
    for g in np.flatnonzero(words[:, 0]):
        for b, c in on:
            assert m[g, c] >> b & 1, (g, b, c)
        if off is not None:
            assert m[g].any() and (m[g] != (1 << Gp) - 1).any(), g


# ---- 1. slot counts around the group kernel's trips -------------------------------------------------------------------

def slot_case(nfft, Gp, C_, nframes=3):
    """-> (x, starts, offset, pairs, R, on, off)"""
    def make():
        rng = np.random.default_rng(6000 + nfft + 37 * Gp + C_)
        R = slot_nrep(nfft, Gp * C_)
        pairs = pair_table(rng, nfft, Gp, C_, R)
        on, off = planted_slots(rng, Gp, C_)
        return windows(rng, nfft, pairs, nframes, on) + (pairs, R, on, off)
    return cached(("slots", nfft, Gp, C_, nframes), make)


@pytest.mark.parametrize("nfft", SLOT_NFFT)
@pytest.mark.parametrize("shape", SLOT_SHAPES, ids=lambda s: "%dx%d" % s)
def test_slot_cases(V, shape, nfft):
    """the slot counts are the published sizes' neighbours, the comb loop makes 2, 2 and 4 trips at C 257, 512 and 1024,
    the full tables at 2048 give the spectrum kernel's slot loop 4 trips over every bin, and with 32 groups bit 31 of a
    mask is set in one comb and clear in another"""
    geo = V.TII_GEOMETRY
    T, S = geo["group_threads"], geo["slots_max"]
    assert sorted({g * c for g, c in SLOT_SHAPES}) == [T - 1, T, T + 1, 3 * T + 3, S - 1, S]
    assert max(g for g, _ in SLOT_SHAPES) == geo["groups_max"] and [-(-c // T) for c in (257, 512, 1024)] == [2, 2, 4]
    Gp, C_ = shape
    x, starts, offset, pairs, R, on, off = slot_case(nfft, Gp, C_)
    if nfft == 2048 and Gp * C_ in (T, S):
        assert 2 * R * Gp * C_ == nfft and -(-Gp * C_ // (nfft // 8)) == (4 if Gp * C_ == S else 1)
    assert 1 <= R <= geo["nrep_max"] and 2 * R * Gp * C_ <= nfft
    p = Tii(nfft, Gp, C_, R, navg=2, thr=2.5, offset=offset)
    samples, mfmt = as_format(x, IQ_F32)
    words, energy = tii_model(samples, starts, p, pairs, twiddles_model(nfft))
    assert words[:, 0].tolist() == [2, 1]
    check_masks(words, Gp, on, off)
    m = masks_of(words)
    if Gp == 32:
        assert (m[:, 0] >> 31 == 1).all() and (m[:, 1:] >> 31 == 0).any()
    if Gp > 8:
        assert (m & 0xFFFFFF00).any()  # bits 8 and up


# ---- 2. navg at its cap ---------------------------------------------------------------------------------------------------

NAVG_SKIPPED = (0, 1, 255, 256)


def navg_case():
    """513 frames at nfft 64, start -1 at frames 0, 1, 255 and 256 -> (x, starts, offset, pairs, on, off)"""
    def make():
        nfft, Gp, C_, R = NAVG_SHAPE
        rng = np.random.default_rng(6100)
        pairs = random_pairs(rng, nfft, Gp, C_, R)
        on, off = {(3, 0), (0, 2), (2, 1)}, (3, 2)
        x, starts, offset = windows(rng, nfft, pairs, 513, on)
        starts[list(NAVG_SKIPPED)] = -1
        return x, starts, offset, pairs, on, off
    return cached("navg", make)


def navg_nused(navg, nframes):
    return [sum(1 for t in range(g, min(g + navg, nframes)) if t not in NAVG_SKIPPED) for g in range(0, nframes, navg)]


@pytest.mark.parametrize("navg,nframes", NAVG_RUNS)
def test_navg_cases(V, navg, nframes):
    """full groups at the cap and one below it, a ragged group of one, nused below the group's frame count at both ends of
    the group's list of frames"""
    assert max(n for n, _ in NAVG_RUNS) == V.TII_GEOMETRY["navg_max"]
    nfft, Gp, C_, R = NAVG_SHAPE
    x, starts, offset, pairs, on, off = navg_case()
    p = Tii(nfft, Gp, C_, R, navg=navg, thr=2.5, offset=offset)
    samples, mfmt = as_format(x, IQ_F32)
    words, _ = tii_model(samples, starts[:nframes], p, pairs, twiddles_model(nfft))
    assert words[:, 0].tolist() == navg_nused(navg, nframes)
    assert {256: {257: [253, 0], 513: [253, 255, 1]}, 255: {257: [253, 0], 513: [253, 253, 3]}}[navg][nframes] == words[:, 0].tolist()
    check_masks(words, Gp, on, off)


# ---- 3. odd and tiny slot counts ----------------------------------------------------------------------------------------

def tiny_case(Gp, C_, R):
    def make():
        rng = np.random.default_rng(6200 + 10 * Gp + C_)
        pairs = random_pairs(rng, 64, Gp, C_, R)
        on = {(1, 0)} if (Gp, C_) == (3, 1) else {(2, 0), (0, 4)} if C_ > 1 else {(0, 0)}
        return windows(rng, 64, pairs, 3, on) + (pairs, on)
    return cached(("tiny", Gp, C_, R), make)


@pytest.mark.parametrize("shape", TINY_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_tiny_cases(V, shape):
    """1, 3 and 15 slots: the noise level of one slot is that slot's energy (bit set at thr 1, clear at 2.5); of three, the
    middle one; R = 8 is the cap"""
    Gp, C_, R = shape
    assert max(r for _, _, r in TINY_SHAPES) == V.TII_GEOMETRY["nrep_max"] and 2 * R * Gp * C_ <= 64
    x, starts, offset, pairs, on = tiny_case(*shape)
    samples, mfmt = as_format(x, IQ_F32)
    for thr in (1.0, 2.5):
        words, energy = tii_model(samples, starts, Tii(64, Gp, C_, R, navg=2, thr=thr, offset=offset), pairs, twiddles_model(64))
        noise = words[:, 1].view(F32)
        if Gp * C_ == 1:
            assert np.array_equal(noise, energy.reshape(-1)) and masks_of(words).reshape(-1).tolist() == [int(thr == 1.0)] * 2
        else:
            assert np.array_equal(noise, np.sort(energy.reshape(2, -1), axis=1)[:, (Gp * C_ - 1) // 2])
            if thr == 2.5:
                check_masks(words, Gp, on, off=True)


# ---- 4. ties at the median and at the threshold ---------------------------------------------------------------------------

def tie_case(Gp, C_):
    """GC - 3 distinct pairs for GC slots: the slots TIE_CLASS name one pair, so their energies are equal bit for bit.  Two
    frames, one per group, without noise; every other slot has an amplitude of its own, below (0.2 ... 0.7) or above
    (2 ... 5) the class's 1.0.  Frame 0 has want - 2 slots below: the class holds ranks want - 2 ... want + 1 and slot 9,
    its third, holds the wanted one, with equal slots of lower and higher index.  Frame 1 has one slot fewer below: the
    wanted rank is the class's top one, and the rank above it holds another value -> (x, starts, offset, pairs)"""
    def make():
        GC = Gp * C_
        want = (GC - 1) // 2
        rng = np.random.default_rng(6300 + GC)
        lower = 2 * rng.permutation(31)[:GC - 3] + 2
        others = [s for s in range(GC) if s not in TIE_CLASS]
        table = np.zeros(GC, np.int64)
        table[list(TIE_CLASS)] = lower[0]
        table[others] = lower[1:]
        pairs = table.reshape(1, Gp, C_).astype(np.uint16)
        order = [others[i] for i in rng.permutation(len(others))]
        frames = []
        for nlow in (want - 2, want - 3):
            amps = {s: 1.0 for s in TIE_CLASS[:1]}  # one entry writes the class's pair
            amps.update({s: 0.2 + 0.5 * i / nlow for i, s in enumerate(order[:nlow])})
            amps.update({s: 2.0 + 3.0 * i / (len(order) - nlow) for i, s in enumerate(order[nlow:])})
            frames.append({(s // C_, s % C_): a for s, a in amps.items()})
        return windows(rng, 64, pairs, 2, frames, noise=0.0) + (pairs,)
    return cached(("tie", Gp, C_), make)


THR_AT, THR_ABOVE = 1.0, float(np.nextafter(F32(1.0), F32(2.0)))


def decide_variant(E, thr, rank_up=0, strict=False, tie_break=True):
    """decide_model with one rule changed: the rank above the lower median's, v > tau for v >= tau, or a rank that counts
    smaller values only (then no slot may have the wanted rank: the level stays 0)"""
    v = E.reshape(-1)
    want = (v.size - 1) // 2 + rank_up
    if tie_break:
        noise = rank_select(v, want)
    else:
        rank = (v[None, :] < v[:, None]).sum(axis=1)
        noise = v[rank == want][0] if (rank == want).any() else F32(0)
    tau = F32(thr) * noise
    on = (E > 0) & ((E > tau) if strict else (E >= tau))
    mask = np.zeros(E.shape[1], np.uint32)
    for b in range(E.shape[0]):
        mask |= on[b].astype(np.uint32) << np.uint32(b)
    return noise, mask


@pytest.mark.parametrize("shape", TIE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_tie_cases(shape):
    """in float32 and in every integer format: four slots equal the noise level bit for bit; at thr 1.0 their bits are set,
    at the next float clear; the upper-rank, the strictly-greater and the tie-blind variants of the decision each give
    another answer"""
    Gp, C_ = shape
    GC = Gp * C_
    want = (GC - 1) // 2
    x, starts, offset, pairs = tie_case(Gp, C_)
    cls = list(TIE_CLASS)
    for fmt in (IQ_F32,) + INT_FORMATS:
        samples, mfmt = as_format(x, fmt)
        p = Tii(64, Gp, C_, 1, navg=1, thr=THR_AT, offset=offset)
        words, energy = tii_model(samples, starts, p, pairs, twiddles_model(64), fmt=mfmt)
        above = tii_model(samples, starts, Tii(64, Gp, C_, 1, navg=1, thr=THR_ABOVE, offset=offset), pairs, twiddles_model(64), fmt=mfmt)[0]
        for g in range(2):
            v = energy[g].reshape(-1)
            noise = words[g, 1:2].view(F32)[0]
            assert (v[cls] == noise).all() and (v == noise).sum() == 4 and noise > 0 and np.unique(v).size == GC - 3
            idx = np.arange(GC)
            rank = np.array([((v < v[s]) | ((v == v[s]) & (idx < s))).sum() for s in range(GC)])
            holder = int(np.flatnonzero(rank == want)[0])
            assert holder == (cls[2], cls[3])[g]
            bits = np.array([masks_of(words)[g, s % C_] >> (s // C_) & 1 for s in range(GC)])
            bits_above = np.array([masks_of(above)[g, s % C_] >> (s // C_) & 1 for s in range(GC)])
            assert np.array_equal(bits, v >= noise) and np.array_equal(bits_above, v > noise) and bits[cls].all()
            assert 0 < bits_above.sum() < bits.sum() < GC
            ref = decide_model(energy[g], THR_AT)
            assert ref[0] == noise and np.array_equal(ref[1], masks_of(words)[g])
            up = decide_variant(energy[g], THR_AT, rank_up=1)
            assert (up[0] != noise) == (g == 1) and (g == 0 or not np.array_equal(up[1], ref[1]))
            assert not np.array_equal(decide_variant(energy[g], THR_AT, strict=True)[1], ref[1])
            blind = decide_variant(energy[g], THR_AT, tie_break=False)
            assert blind[0] == 0 and not np.array_equal(blind[1], ref[1])
            same = decide_variant(energy[g], THR_AT)
            assert same[0] == ref[0] and np.array_equal(same[1], ref[1])


# ---- 5. independence from the launch ------------------------------------------------------------------------------------

LAUNCH_SHAPE = (2048, 32, 32)


def test_launch_case():
    """group 0 of five groups of one frame equals the only group of a call with one frame, at 1024 slots"""
    nfft, Gp, C_ = LAUNCH_SHAPE
    x, starts, offset, pairs, R, on, off = slot_case(nfft, Gp, C_, nframes=5)
    p = Tii(nfft, Gp, C_, R, navg=1, thr=2.5, offset=offset)
    samples, mfmt = as_format(x, IQ_F32)
    w5, e5 = tii_model(samples, starts, p, pairs, twiddles_model(nfft))
    w1, e1 = tii_model(samples, starts[:1], p, pairs, twiddles_model(nfft))
    assert np.array_equal(w5[:1], w1) and np.array_equal(e5[:1].view(np.uint32), e1.view(np.uint32))
    assert len({w.tobytes() for w in w5}) == 5


def test_geometry_is_published(V):
    g = V.TII_GEOMETRY
    assert set(g) >= {"group_threads", "slots_max", "groups_max", "navg_max", "nrep_max"}
    assert all(isinstance(v, int) and v > 0 for v in g.values())
    assert g["navg_max"] <= g["group_threads"] and g["slots_max"] % g["group_threads"] == 0 and g["groups_max"] == 32
