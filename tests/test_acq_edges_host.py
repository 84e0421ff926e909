"""CPU-only: the inputs of tests/test_gpu_acq_edges.py - vit_ofdm_acquire_dev at the caps and edges of its geometry - and
the conditions under which they mean something, checked with acquire_model (tests/test_acq_host.py) alone.  The kernels'
partition sizes come from ACQ_GEOMETRY of the package, so a retuned kernel moves these cases with it:

  power    every block length in every format, the block count placed around the wavefront's tile of chunks;
  windows  Ln, Lr at their cap, a period's candidate count around the LDS tile, set by Pb and by the end of the stream;
  ties     the last minimum at an LDS tile edge, held by a thread that has met an equal q before;
  periods  one candidate per period, a last period of one, nperiods at and past nblk // Pb;
  thr      q <= thr at equality and one float below.

Out of scope, and not forgotten: the second trip of either kernel's grid stride.  The power kernel makes one beyond 8192
workgroups of 4 wavefronts of 4 KiB (128 MiB of samples), the search beyond 2^20 periods that hold candidates; neither fits
a test of a few seconds with a Python model, and both loops are plain strides that carry no state."""
import numpy as np
import pytest

from test_acq_host import NONE, Acq, acquire_model, window_sums_model
from test_fft_host import F32
from test_iqfmt_host import INT_FORMATS, IQ_CS8, IQ_CS16, IQ_CU8, convert_model, quantise

IQ_F32 = 0
FORMATS = (IQ_F32,) + INT_FORMATS
SAMPLE_BYTES = {IQ_F32: 8, IQ_CU8: 2, IQ_CS8: 2, IQ_CS16: 4}
BLOCKS = (8, 16, 32, 64, 128, 256, 512)
WINDOWS = ("cap", "cap"), ("cap", 1), (1, "cap")  # (Ln, Lr), "cap" = ACQ_GEOMETRY["window_max"]
COUNTS = ("1", "T-1", "T", "T+1", "2T", "2T+1")   # a period's candidates, T = ACQ_GEOMETRY["search_tile"]
TIE_TARGETS = (-1, 0, 1)                          # the last minimum is candidate T + d of its period
TIE_FORMATS = (IQ_F32, IQ_CS8, IQ_CS16)           # exact zeros: no CU8 sample is zero
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def as_format(x, fmt):
    """-> (what the device gets: complex64 (n,) or raw (n, 2), the floats of the definition, scale)"""
    if fmt == IQ_F32:
        f = np.asarray(x, np.complex64)
        return f, f, 1.0
    raw, scale = quantise(x, fmt)
    return raw, convert_model(raw, fmt, scale), scale


def poisoned(dev, floats, fmt, nsamples):
    """both images with everything at and beyond nsamples replaced - NaN, or the codes' complements: a sample read from
    there changes a word"""
    dev, floats = dev.copy(), floats.copy()
    if fmt == IQ_F32:
        dev[nsamples:] = complex(np.nan, np.nan)
        floats[nsamples:] = complex(np.nan, np.nan)
    else:
        dev[nsamples:] = ~dev[nsamples:]
        floats[nsamples:] = complex(np.nan, np.nan)  # the model must not read them either
    return dev, floats


def gaussian(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5)


def put_null(x, B, Ln, j, depth):
    """a null that ends in the middle of block j (counted from sample 0) and covers the Ln blocks in front of it whole,
    wherever `first` < B/2 puts the block edges"""
    edge = j * B + B // 2
    assert edge - (Ln + 1) * B >= 0
    x[edge - (Ln + 1) * B:edge] *= depth


def q_of(floats, a, nsamples=None):
    """q of every candidate, by the model's own parts"""
    _, _, p = acquire_model(floats, a, 1, nsamples=nsamples)
    ncand = max(p.size - a.Lr - a.Ln + 1, 0)
    N, R = window_sums_model(p, a.Ln, 0, ncand), window_sums_model(p, a.Lr, a.Ln, ncand)
    with np.errstate(all="ignore"):
        return np.where(R > 0, N / np.where(R > 0, R, F32(1)), F32(np.inf)).astype(F32)


def choose(qk, rule, tile):
    """the candidate a period's search returns under the definition ("last") and under two wrong ones"""
    last_min = lambda v: v.size - 1 - int(np.argmin(v[::-1]))  # noqa: E731
    if rule == "last":
        return last_min(qk)
    if rule == "first":
        return int(np.argmin(qk))
    lo = (qk.size - 1) // tile * tile  # "last_tile": what a search that forgets the tiles before the last returns
    return lo + last_min(qk[lo:])


# ---- 1. every block length in every format ---------------------------------------------------------------------------

def power_lg(B, fmt, geo):
    chunks = B * SAMPLE_BYTES[fmt] // geo["chunk_bytes"]
    assert chunks >= 1 and chunks & (chunks - 1) == 0
    return chunks.bit_length() - 1


def power_nblks(lg, geo):
    """block counts whose chunk count nblk << lg lies around the wavefront's tile: one block less, the tile, one block
    more, three tiles and a part; a block of half a tile: odd and even counts; a block of a tile: 1, 2 and 5"""
    bpt = geo["tile_chunks"] >> lg
    assert bpt >= 1
    if bpt >= 4:
        return [bpt - 1, bpt, bpt + 1, 3 * bpt + bpt // 2 + 1]
    return [1, 2, 3, 7, 8] if bpt == 2 else [1, 2, 5]


def power_case(B, fmt, nblk):
    """-> (dev, floats, scale, nsamples, the null's block or None): nblk blocks from first = 0 and from first = 1, the
    stream ending in mid-block, 2B + 5 poisoned samples behind it"""
    def make():
        rng = np.random.default_rng(1000 + 8 * B + fmt + 64 * nblk)
        n = 1 + nblk * B + B // 2 + 2
        x = gaussian(rng, n + 2 * B + 5)
        j = None
        if nblk >= 5:
            j = nblk // 2 + 1
            put_null(x, B, 2, j, 0.01)
        dev, floats, scale = as_format(x, fmt)
        dev, floats = poisoned(dev, floats, fmt, n)
        return dev, floats, scale, n, j
    return cached(("power", B, fmt, nblk), make)


def power_acq(B, nblk, first):
    return Acq(B, 2, 1, max(nblk, 1), first=first, offset=B // 2 - 7)


@pytest.mark.parametrize("B", BLOCKS)
def test_power_cases(V, B):
    """the 28 cells: lg runs 0 ... 8 over them, the chunk counts sit at the tile's edges, and wherever the stream is long
    enough for a null the model finds it at a candidate that is neither the period's first nor its last"""
    geo = V.ACQ_GEOMETRY
    for fmt in FORMATS:
        lg = power_lg(B, fmt, geo)
        counts = power_nblks(lg, geo)
        chunks = [c << lg for c in counts]
        T = geo["tile_chunks"]
        if lg < 7:
            assert chunks[:3] == [T - (1 << lg), T, T + (1 << lg)] and 3 * T < chunks[3] < 4 * T
        elif lg == 7:
            assert any(c % 2 for c in counts) and any(c % 2 == 0 for c in counts) and min(chunks) < T < max(chunks)
        else:
            assert lg == 8 and chunks[0] == T
        found = 0
        for nblk in counts:
            dev, floats, scale, n, j = power_case(B, fmt, nblk)
            for first in (0, 1):
                assert (n - first) // B == nblk and (n - first) % B  # ends in mid-block
                start, info, p = acquire_model(floats, power_acq(B, nblk, first), 2, nsamples=n)
                assert p.size == nblk and np.isfinite(p).all() and info[1, 0] == NONE
                if j is not None:
                    assert info[0, 0] not in (NONE, 0, nblk - 3) and start[0] != -1
                    found += 1
        assert found >= 2
    assert sorted({power_lg(b, f, geo) for b in BLOCKS for f in FORMATS}) == list(range(9))


# ---- 2. windows at their cap, candidate counts around the LDS tile ----------------------------------------------------

def window_case(win, count, way, geo):
    """-> (x complex128, Acq, nperiods, k: the period with the null, ncand of period k).  way "pb": Pb is the count, two
    whole periods, a third of at most 3 candidates and a fourth of none; way "end": a period of two tiles and a part,
    then the stream ends so that the second period holds the count.  The null, 60 dB deep, ends at the last candidate but
    one of period k; a period of one or two candidates has no such place (way "pb": the null lies there all the same; way
    "end": it lies in the long period in front).  Neighbouring periods' windows overlap wherever Pb < Ln + Lr: the
    expected words are the model's"""
    def make():
        T, cap = geo["search_tile"], geo["window_max"]
        Ln, Lr = (cap if w == "cap" else w for w in win)
        c = {"1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "2T": 2 * T, "2T+1": 2 * T + 1}[count]
        B = 8
        if way == "pb":
            Pb, nper = c, 4
            nblk = 2 * Pb + Ln + Lr - 1 + min(c, 3)
            k, i = 1, max(c - 2, 0)
            nk = c
        else:
            Pb, nper = 2 * T + 904, 3
            nblk = Pb + Ln + Lr - 1 + c
            k, i, nk = (1, c - 2, c) if c >= 3 else (0, Pb - 2, Pb)
        rng = np.random.default_rng(2000 + c + 7 * Ln + 3 * Lr + (way == "pb"))
        x = gaussian(rng, nblk * B + 5)
        put_null(x, B, Ln, Ln + k * Pb + i, 0.001)
        return x, Acq(B, Ln, Lr, Pb), nper, k, nk
    return cached(("window", win, count, way), make)


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("win", WINDOWS, ids=lambda w: "%s-%s" % w)
def test_window_cases(V, win, count):
    """each way gives the count it is named for, a full tile under two capped windows fills the LDS to one float short of
    its size, and the model finds the null: accepted, and (where the period has three candidates) at neither end"""
    geo = V.ACQ_GEOMETRY
    T, cap = geo["search_tile"], geo["window_max"]
    for way, fmt in (("pb", IQ_F32), ("end", IQ_CS16)):
        x, a, nper, k, nk = window_case(win, count, way, geo)
        floats = as_format(x, fmt)[1]
        start, info, p = acquire_model(floats, a, nper)
        ncand = p.size - a.Ln - a.Lr + 1
        per_period = [min(max(ncand - j * a.Pb, 0), a.Pb) for j in range(nper)]
        want = {"1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "2T": 2 * T, "2T+1": 2 * T + 1}[count]
        assert per_period[k] == nk and want in per_period and per_period[-1] == 0 and info[-1, 0] == NONE
        assert per_period[1] == want
        assert (info[:-1, 0] != NONE).all() and start[k] != -1
        if nk >= 3:
            assert 0 < info[k, 0] < nk - 1
    assert max(a.Ln, a.Lr) == cap
    if win == ("cap", "cap"):
        assert T + a.Ln + a.Lr - 1 == T + 2 * cap - 1  # a full tile and its halo: all but one float of the search's LDS


# ---- 3. the last minimum at an LDS tile edge ------------------------------------------------------------------------

TIE_COMB = 300  # tied candidates, 3 apart: 897 candidates from the first to the last, more than 3 * 256


def tie_case(d, geo):
    """-> (x complex128, Acq, nperiods, k, target).  Period 1 of two tiles and a part.  Candidates target - 3m, m < 300,
    have two all-zero blocks in front and a block of signal behind: q = 0 exactly, 300 times, the last at target = T + d.
    Three candidates apart, so a thread of 256 meets a tie again after 768 candidates, inside a tile and across the edge.
    A null 20 dB deep lies in the tile before (candidate 1000) and in the tile behind (T + T + 400): a strictly smaller
    q in front of the later tile's minimum, and no q = 0 behind the edge's tile."""
    def make():
        T = geo["search_tile"]
        B, Ln, Lr, Pb = 8, 2, 1, 2 * T + 904
        nblk = 2 * Pb + Ln + Lr - 1 + 3
        rng = np.random.default_rng(3000 + d)
        x = gaussian(rng, nblk * B + 5)
        target = T + d
        j = Ln + Pb + target
        assert 3 * TIE_COMB < target - 1000 and 2 * T + 400 < Pb
        for m in range(TIE_COMB):
            x[(j - 3 * m - 2) * B:(j - 3 * m) * B] = 0
        x[j * B:j * B + 3] = 0
        for i in (1000, 2 * T + 400):
            put_null(x, B, Ln, Ln + Pb + i, 0.1)
        return x, Acq(B, Ln, Lr, Pb), 3, 1, target
    return cached(("tie", d), make)


@pytest.mark.parametrize("fmt", TIE_FORMATS)
@pytest.mark.parametrize("d", TIE_TARGETS)
def test_tie_cases(V, d, fmt):
    """the model returns the target with q = 0; the first minimum and the minimum of the last tile alone are other
    candidates; the ties span more than three strides of the search's threads"""
    geo = V.ACQ_GEOMETRY
    T = geo["search_tile"]
    x, a, nper, k, target = tie_case(d, geo)
    floats = as_format(x, fmt)[1]
    start, info, _ = acquire_model(floats, a, nper)
    assert info[k, 0] == target and info[k, 1] == 0 and start[k] != -1 and (info[:, 0] != NONE).all()
    qk = q_of(floats, a)[k * a.Pb:(k + 1) * a.Pb]
    assert qk.size == a.Pb and choose(qk, "last", T) == target
    ties = np.flatnonzero(qk == 0)
    assert ties.size == TIE_COMB and ties[-1] == target and (np.diff(ties) == 3).all()
    assert choose(qk, "first", T) == target - 3 * (TIE_COMB - 1) != target
    assert choose(qk, "last_tile", T) not in (target, choose(qk, "first", T))
    assert 0 < qk[2 * T:].min() <= qk[2 * T + 400] < 0.5 and 0 < qk[1000] < 0.5  # the shallow nulls are there and are no ties


# ---- 4. period geometry -----------------------------------------------------------------------------------------------

def single_candidate_case(fmt):
    """Pb = 1: 300 periods of one candidate each, exactly -> (dev, floats, scale, Acq, the null's period)"""
    def make():
        B, Ln, Lr = 8, 2, 1
        nblk = 300 + Ln + Lr - 1
        x = gaussian(np.random.default_rng(4000), nblk * B + 5)
        put_null(x, B, Ln, 150, 0.01)
        return as_format(x, fmt) + (Acq(B, Ln, Lr, 1), 150 - Ln)
    return cached(("single", fmt), make)


GUARD_PB = 48
GUARD_NBLK = (3 * GUARD_PB, 3 * GUARD_PB + 2, 3 * GUARD_PB + 3)  # period 3: no candidate, none still, exactly one


def guard_case(fmt):
    """Pb = 48, Ln 2, Lr 1 -> (dev, floats, scale, Acq): 147 blocks and a part, the null's edge in block 146, which is
    period 3's only candidate when all 147 blocks count; cut to 144 or 146 blocks period 3 = nblk // Pb has none"""
    def make():
        B, Ln, Lr = 8, 2, 1
        x = gaussian(np.random.default_rng(4001), GUARD_NBLK[-1] * B + 5)
        put_null(x, B, Ln, 3 * GUARD_PB + Ln, 0.01)
        put_null(x, B, Ln, GUARD_PB + 20, 0.01)
        return as_format(x, fmt) + (Acq(B, Ln, Lr, GUARD_PB),)
    return cached(("guard", fmt), make)


def test_period_cases():
    inf = np.array([np.inf], F32).view(np.uint32)[0]
    for fmt in (IQ_F32, IQ_CU8):
        dev, floats, scale, a, k = single_candidate_case(fmt)
        start, info, p = acquire_model(floats, a, 302)
        assert p.size == 302 and (info[:300, 0] == 0).all() and (info[300:, 0] == NONE).all()
        assert start[k] != -1 and (start[300:] == -1).all()
        dev, floats, scale, a = guard_case(fmt)
        for nblk in GUARD_NBLK:
            n = nblk * a.B + 5
            assert nblk // a.Pb == 3
            for nper in (3, 4, 5):  # nblk // Pb, one and two more: k <= nblk / Pb at equality and past it
                start, info, p = acquire_model(floats, a, nper, nsamples=n)
                assert p.size == nblk and (info[:3, 0] != NONE).all() and 0 < info[1, 0] < a.Pb - 1 and start[1] != -1
                if nper > 3:
                    one = nblk == GUARD_NBLK[-1]
                    assert (info[3, 0] == 0 and start[3] != -1) if one else (info[3].tolist() == [NONE, inf, 0, 0])
                if nper > 4:
                    assert info[4].tolist() == [NONE, inf, 0, 0] and start[4] == -1


# ---- 5. the threshold at equality -------------------------------------------------------------------------------------

def threshold_case(fmt):
    """three periods of 40 blocks of 32 with a null 40 dB deep in each -> (dev, floats, scale, Acq without thr)"""
    def make():
        B, Ln, Lr, Pb = 32, 5, 3, 40
        rng = np.random.default_rng(5000)
        x = gaussian(rng, (3 * Pb + Ln + Lr) * B + B // 2 + 3)
        for k in range(3):
            put_null(x, B, Ln, Ln + k * Pb + 10 + 7 * k, 0.01)
        return as_format(x, fmt) + (Acq(B, Ln, Lr, Pb, offset=-9),)
    return cached(("thr", fmt), make)


def threshold_pair(floats, a, k=1):
    """-> (thr equal to period k's q, the next float below it), both from the model's info word"""
    q = acquire_model(floats, a, 3)[1][k, 1:2].view(F32)[0]
    assert 0 < q < 0.01
    return float(q), float(np.nextafter(q, F32(0)))


def with_thr(a, thr):
    return Acq(a.B, a.Ln, a.Lr, a.Pb, thr=thr, first=a.first, offset=a.offset)


def test_threshold_cases():
    for fmt in (IQ_F32, IQ_CU8):
        dev, floats, scale, a = threshold_case(fmt)
        at, below = threshold_pair(floats, a)
        assert F32(at) == at and F32(below) == below and below < at
        s_at, i_at, _ = acquire_model(floats, with_thr(a, at), 3)
        s_below, i_below, _ = acquire_model(floats, with_thr(a, below), 3)
        assert s_at[1] != -1 and s_below[1] == -1 and np.array_equal(i_at, i_below)
        assert 0 < i_at[1, 0] < a.Pb - 1 and len({int(v) for v in i_at[:, 1]}) == 3  # the other periods' q differ


def test_geometry_is_published(V):
    """the constants the cases are built from: positive integers, a tile of whole wavefront rows, an LDS that holds a
    tile and two windows"""
    g = V.ACQ_GEOMETRY
    assert set(g) >= {"chunk_bytes", "tile_chunks", "search_tile", "window_max"}
    assert all(isinstance(v, int) and v > 0 for v in g.values())
    assert g["tile_chunks"] % 64 == 0 and g["chunk_bytes"] == 16 and g["window_max"] == 4096
    assert (g["search_tile"] + 2 * g["window_max"]) * 4 + 64 <= 64 * 1024
