"""Merge-directed frames for the block-parallel tracebacks of csrc/vit_pk.hip and csrc/vit_lat.hip: the decision history of
a frame (oracle.decisions: the words ChainBack itself consumes), models of the four traceback forms on that history, and
seeded generators whose frames are KEPT BY WHAT THE MODEL SAYS THEY DO - which block misses, how deep a re-trace cascade
runs, which in-flight part fails its check, where a wave gives up - instead of hoping that noise takes each path.

No GPU and no product library here: numpy, and the oracle for the decision words.  tests/test_tb_paths_host.py asserts
the models (their decoded bits ARE the oracle's) and the class counts; tests/test_gpu_tb_paths.py runs the frames through
the kernels and compares the -DVIT_DIAG_SPEC counters with the models' totals.

Geometry, restated from the kernel sources (T = framebits + 6 trellis steps, step t decodes bit t - 6, steps 0..5 are never
traced; a state is ChainBack's E >> 2, one step back is S' = (S >> 1) | (k << 5) with k = bit S of dec[t]; the kernels'
positions P / L are bijections of S at a given t, so equality of positions is equality of states):

  fast form (traceback_part16; waves of four equally long frames of a multiple of 16 bits): parts of 256 steps cut from
    the top, part p = [lo, hi), hi = T - 256 p, lo = max(hi - 256, 6) = 6 mod 16, nl = (hi - lo) / 16 lanes per frame, lane
    q = the 16 steps from lo + 16 q.  The two top lanes start at the part's top from the true position (the second one
    walks the top block first); the others start 30 steps above their block (index 45) from state 0.  A lane whose
    position at its block's top differs from what the lane above ended in re-traces its block; passes repeat (bound 17)
    until no lane of the WAVE changes.
  in-flight form (<SPEC>, long-frame kernel, NP = ceil(fb / 256) > 1): during the forward pass parts NP-1 .. 1 are traced
    with EVERY lane speculative and the top lane trusted; spec(p) = the top lane's position at the part's top, out(p) =
    lane 0's end position; misses = lanes of all four frames that change in pass 0.  misses >= 8 at a part p >= 2: the
    wave gives up, parts p-1 .. 1 stay untraced.  After the forward pass part 0 is traced from state 0 (fast form), then
    the chain loop re-traces, top-down, the topmost part whose spec (four frames as one word) is not the out of the part
    above (an untraced part never matches), from that out, with the fast form; at most NP iterations.
  general form (traceback_part; any other wave): nb = ceil(Tmax / 16) blocks, the top part starts at block R = max(nb - 17,
    0) (ts = max(16 R, 6)), then groups of 16 blocks downwards.  Per part: span = te_max - ts over the wave's longest
    frame, BL = 5 ceil(span / 80), 16 lanes per frame, lane q = BL steps from ts + q BL, i_last = te - 1 - tbase for the
    lane's own frame, fixed = i_last <= BL - 1 + warm (starts at the frame's last step of the part from the position the
    part above ended in, state 0 at a frame's end); the others start at index BL - 1 + warm from state 0.  warm = 30 until
    a pass-0 ballot over the wave's 64 lanes shows >= 8 misses, 90 for the parts that follow.  Pass bound 17.
  latency kernel (vit_lat.hip): one frame per wave, one part, 64 lanes, BL = 6 ceil(fb / 384), warm-up 30, pass bound 65.
"""
import os

import numpy as np

M64 = (1 << 64) - 1
TAIL = 6
HARD_MISSES = 8
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TB_PATHS_NPY = os.path.join(GOLD, "reference_tb_paths.npy")
SHORT_MAX = 778  # the longest frame of the single-segment kernel

_ONE, _FIVE = np.uint64(1), np.uint64(5)


# ---- walking the decision history ------------------------------------------------------------------------------------
def _walk(dec, S, t_top, n, live=None):
    """every lane: from state S[i] before step t_top[i], n steps back (t_top, t_top - 1, ...); lanes step only where
    live[i, j] -> (S after, k[i, j] = the bit of step t_top[i] - j)"""
    S = np.asarray(S, np.uint64).copy()
    t_top = np.asarray(t_top, np.int64)
    ks = np.zeros((S.size, n), np.uint8)
    for j in range(n):
        t = t_top - j
        on = (t >= 0) & (t < dec.size) if live is None else live[:, j]
        k = (dec[np.clip(t, 0, dec.size - 1)] >> S) & _ONE
        S = np.where(on, (S >> _ONE) | (k << _FIVE), S)
        ks[:, j] = np.where(on, k, 0)
    return S, ks


def serial_chainback(dec, fb):
    """ChainBack (deconvolve.cpp:416-435) on the decision words -> (decoded bits fb, state before every step: fb + 7 values)"""
    S, bits, st = 0, np.zeros(fb, np.uint8), np.zeros(fb + TAIL + 1, np.int64)
    d = [int(x) for x in dec]
    for t in range(fb + TAIL - 1, TAIL - 1, -1):
        st[t + 1] = S
        k = (d[t] >> S) & 1
        S = (S >> 1) | (k << 5)
        bits[t - TAIL] = k
    st[TAIL] = S
    return bits, st


def pack_bits(bits):
    """decoded bits -> output bytes, MSB first, a partial last byte padded with zero bits"""
    return np.packbits(np.asarray(bits, np.uint8), bitorder="big")


def numpy_acs(sym, ge=False):
    """self-check of the decision words: the trellis of deconvolve.cpp in plain numpy (short frames only)"""
    sym = np.asarray(sym, np.int64).reshape(-1, 4)
    i = np.arange(32)
    par = lambda x: np.array([bin(int(v)).count("1") & 1 for v in x])  # noqa: E731
    mask = np.stack([par((2 * i) & p) * 255 for p in (109, 79, 83, 109)])
    avg = lambda a, b: (a + b + 1) >> 1  # noqa: E731
    old = np.full(64, 63)
    old[0] = 0
    out = np.zeros(sym.shape[0], np.uint64)
    for t in range(sym.shape[0]):
        x = sym[t][:, None] ^ mask
        metric = avg(avg(x[0], x[1]), avg(x[2], x[3])) >> 2
        mm = 63 - metric
        m0, m1 = np.minimum(old[:32] + metric, 255), np.minimum(old[32:] + mm, 255)
        m2, m3 = np.minimum(old[:32] + mm, 255), np.minimum(old[32:] + metric, 255)
        d0, d1 = m1 <= m0, m3 <= m2
        new = np.empty(64, np.int64)
        new[0::2], new[1::2] = np.where(d0, m1, m0), np.where(d1, m3, m2)
        w = 0
        for s in range(32):
            w |= (int(d0[s]) << (2 * s)) | (int(d1[s]) << (2 * s + 1))
        out[t] = w
        if t & 1 and (new[0] >= 150 if ge else new[0] > 150):
            new = np.maximum(new - 63, 0)
        old = new
    return out


# ---- one frame's share of a part --------------------------------------------------------------------------------------
class PartTrace:
    """what one frame's lanes did in one part: miss[pass] = lanes that re-traced in that pass, out = end state, spec = (in
    flight) the top lane's state at the part's top, bits[lo - 6 ...] = decoded bits of the part"""
    __slots__ = ("miss", "out", "spec", "bits", "lo", "nspec")

    @property
    def depth(self):
        return len(self.miss)


def fast_part(dec, lo, nl, S_top, spec=False):
    q = np.arange(nl)
    tbase = lo + 16 * q
    fixed = np.zeros(nl, bool) if spec else (nl - q) <= 2
    P_in = np.zeros(nl, np.uint64)
    sp = ~fixed
    if sp.any():
        P_in[sp], _ = _walk(dec, np.zeros(int(sp.sum()), np.uint64), tbase[sp] + 45, 30)
    if not spec:
        P_in[nl - 1] = S_top
        if nl >= 2:
            P_in[nl - 2] = _walk(dec, [S_top], [tbase[nl - 2] + 31], 16)[0][0]
    P_out, ks = _walk(dec, P_in, tbase + 15, 16)
    r = PartTrace()
    r.miss, r.lo, r.nspec = [], lo, int(sp.sum())
    for _ in range(17):
        new_in = np.empty(nl, np.uint64)
        new_in[:-1] = P_out[1:]
        new_in[-1] = P_in[-1] if spec else S_top
        ch = ~fixed & (new_in != P_in)
        if not ch.any():
            break
        r.miss.append(np.flatnonzero(ch))
        P_in[ch] = new_in[ch]
        P_out[ch], ks[ch] = _walk(dec, P_in[ch], tbase[ch] + 15, 16)
    else:
        raise AssertionError("fast form: pass bound reached")
    r.out, r.spec = int(P_out[0]), int(P_in[-1])
    r.bits = ks[:, ::-1].reshape(-1)  # lane q: steps tbase .. tbase + 15
    return r


def block_part(dec, ts, te, BL, nlanes, S_top, warm):
    """general form / latency kernel, one frame's lanes of one part -> (PartTrace, fixed lanes).  State before a pass loop
    only: the loop itself runs per wave (general_wave) because the warm-up switch is a ballot over the wave."""
    q = np.arange(nlanes)
    tbase = ts + q * BL
    work = tbase < te
    i_last = np.where(work, te - 1 - tbase, 0)
    q_top = (te - 1 - ts) // BL if te > ts else 0
    i_warm = BL - 1 + warm
    i_start = np.minimum(i_last, i_warm)
    fixed = work & (i_last <= i_warm)
    P = np.where(fixed, S_top, 0).astype(np.uint64)
    nw = i_warm - BL + 1
    ii = i_warm - np.arange(nw)
    P_in, _ = _walk(dec, P, tbase + i_warm, nw, live=work[:, None] & (ii[None, :] <= i_start[:, None]))
    io = BL - 1 - np.arange(BL)
    live = work[:, None] & (io[None, :] <= i_start[:, None])
    P_out, ks = _walk(dec, P_in, tbase + BL - 1, BL, live=live)
    P_out = np.where(work, P_out, S_top).astype(np.uint64)
    return dict(tbase=tbase, work=work, q_top=q_top, fixed=fixed, P_in=P_in, P_out=P_out, ks=ks, live=live, BL=BL, S_top=S_top, ts=ts, te=te)


def block_pass(dec, f):
    """one pass of the check for one frame's lanes -> lanes that change (not yet re-traced)"""
    n = f["P_out"].size
    new_in = np.full(n, f["S_top"], np.uint64)
    below = np.arange(n) < f["q_top"]
    new_in[:-1] = np.where(below[:-1], f["P_out"][1:], new_in[:-1])
    f["new_in"] = new_in
    return f["work"] & ~f["fixed"] & (new_in != f["P_in"])


def block_retrace(dec, f, ch):
    f["P_in"][ch] = f["new_in"][ch]
    f["P_out"][ch], f["ks"][ch] = _walk(dec, f["P_in"][ch], f["tbase"][ch] + f["BL"] - 1, f["BL"])


def block_bits(f, bits):
    """the part's decoded bits into the frame's bit array"""
    for q in np.flatnonzero(f["work"]):
        k = f["ks"][q][::-1]  # index 0 .. BL - 1
        n = min(f["BL"], f["te"] - int(f["tbase"][q]))
        b0 = int(f["tbase"][q]) - TAIL
        bits[b0:b0 + n] = k[:n]


# ---- a frame and what is known about it ---------------------------------------------------------------------------------
class Frame:
    def __init__(self, fb, sym, dec, tag=""):
        self.fb, self.sym, self.dec, self.tag = fb, sym, dec, tag
        self.T = fb + TAIL
        self._fast, self._true = {}, None

    @property
    def NP(self):
        return (self.fb + 255) >> 8

    def part_range(self, p):
        hi = self.T - 256 * p
        lo = hi - 256 if hi > 256 + TAIL else TAIL
        return lo, hi

    def fast(self, p, S_top, spec=False):
        key = (p, -1 if spec else int(S_top))
        if key not in self._fast:
            lo, hi = self.part_range(p)
            self._fast[key] = fast_part(self.dec, lo, (hi - lo) >> 4, S_top, spec)
        return self._fast[key]

    def true(self):
        if self._true is None:
            self._true = serial_chainback(self.dec, self.fb)
        return self._true


class WaveTrace:
    """what a model says a wave did.  Fields that do not apply to a form stay empty."""

    def __init__(self, form):
        self.form = form
        self.miss0 = {}       # part -> pass-0 misses of the wave (in flight: the in-flight pass)
        self.frame_miss0 = {}  # part -> [lanes of frame k that missed in pass 0]
        self.passes = {}      # part -> re-trace passes the wave ran (the LAST trace of the part)
        self.depth = {}       # part -> per frame: passes in which that frame re-traced
        self.inflight = []    # parts traced in flight, in order
        self.inflight_miss = {}
        self.gave_up_at = None  # the in-flight part whose misses made the wave give up
        self.chain = []       # (part, had been traced in flight) re-traced by the chain loop, in order
        self.chain_frames = []  # per entry of chain: the frames whose recorded top position was not the part above's end
        self.first_ok = []    # parts that passed their check before the part above was re-traced and failed after
        self.warm_switch = []  # general form: parts whose pass 0 switched the wave to warm-up 90
        self.still_miss_90 = 0  # general form: pass-0 misses of parts traced with warm-up 90
        self.fixed90 = 0      # general form: lanes fixed under 90 that would not be under 30
        self.bits = None      # per frame: decoded bits
        self.c = np.zeros(8, np.int64)  # the -DVIT_DIAG_SPEC counters this wave adds


def _fast_serial_part(frames, p, tops, w, bits):
    trs = [f.fast(p, tops[k]) for k, f in enumerate(frames)]
    w.frame_miss0[p] = [t.miss[0] if t.miss else np.zeros(0, np.int64) for t in trs]
    w.miss0[p] = sum(m.size for m in w.frame_miss0[p])
    w.passes[p] = max(t.depth for t in trs)
    w.depth[p] = [t.depth for t in trs]
    w.c[5] += w.miss0[p]
    w.c[6] += w.passes[p]
    for k, t in enumerate(trs):
        bits[k][t.lo - TAIL:t.lo - TAIL + t.bits.size] = t.bits
    return tuple(t.out for t in trs)


def fast_wave_short(frames):
    """single-segment kernel, fast form: every part after the forward pass, top-down"""
    w = WaveTrace("fast")
    w.bits = [np.zeros(f.fb, np.uint8) for f in frames]
    tops = (0, 0, 0, 0)
    for p in range(frames[0].NP):
        tops = _fast_serial_part(frames, p, tops, w, w.bits)
    return w


def fast_wave_long(frames):
    """long-frame kernel, fast form: parts NP-1 .. 1 in flight, part 0, the chain loop"""
    w = WaveTrace("inflight")
    NP = frames[0].NP
    w.bits = [np.zeros(f.fb, np.uint8) for f in frames]
    rec_spec, rec_out = {}, {}
    w.c[0] += 1
    for p in range(NP - 1, 0, -1):
        trs = [f.fast(p, 0, spec=True) for f in frames]
        misses = sum(t.miss[0].size if t.miss else 0 for t in trs)
        w.inflight.append(p)
        w.inflight_miss[p] = (misses, [t.miss[0].size if t.miss else 0 for t in trs])
        rec_spec[p], rec_out[p] = tuple(t.spec for t in trs), tuple(t.out for t in trs)
        for k, t in enumerate(trs):
            w.bits[k][t.lo - TAIL:t.lo - TAIL + t.bits.size] = t.bits
        w.c[1] += 1
        if misses >= HARD_MISSES and p > 1:
            w.c[2] += 1
            w.gave_up_at = p
            break
    rec_spec[0] = (0, 0, 0, 0)
    rec_out[0] = _fast_serial_part(frames, 0, rec_spec[0], w, w.bits)
    ok_at_first = {p for p in range(1, NP) if p in rec_spec and rec_spec[p] == rec_out.get(p - 1)}
    for _ in range(NP):
        bad = [p for p in range(1, NP) if p not in rec_spec or rec_spec[p] != rec_out.get(p - 1)]
        if not bad:
            break
        p = bad[0]
        w.c[3] += 1
        was = p in w.inflight
        w.c[4] += was
        w.chain.append((p, was))
        w.chain_frames.append([k for k in range(4) if p not in rec_spec or rec_spec[p][k] != rec_out[p - 1][k]])
        if p in ok_at_first:
            w.first_ok.append(p)
        rec_spec[p] = rec_out[p - 1]
        rec_out[p] = _fast_serial_part(frames, p, rec_spec[p], w, w.bits)
    else:
        assert all(rec_spec.get(p) == rec_out[p - 1] for p in range(1, NP)), "chain loop: bound reached"
    return w


def general_wave(frames, nlanes=16, lat=False):
    """general form for up to four frames of any lengths (None = an empty slot); lat: the latency kernel's single part"""
    w = WaveTrace("lat" if lat else "general")
    live = [f for f in frames if f is not None]
    Tmax = max(f.T for f in live)
    w.bits = [np.zeros(f.fb, np.uint8) if f is not None else None for f in frames]
    if lat:
        parts = [(TAIL, Tmax)]
    else:
        nb = (Tmax + 15) >> 4
        R = max(nb - 17, 0)
        parts = [(max(16 * R, TAIL), None)]
        g1 = R
        while g1 > 0:
            g0 = max(g1 - 16, 0)
            parts.append((16 * g0 if g0 else TAIL, 16 * g1))
            g1 = g0
    warm, P_part = 30, [0] * len(frames)
    for pi, (ts, tend) in enumerate(parts):
        te_max = Tmax if tend is None else min(Tmax, tend)
        span = te_max - ts
        if span <= 0:
            continue
        BL = 6 * ((frames[0].fb + 383) // 384) if lat else 5 * ((span + 79) // 80)
        fs = []
        for k, f in enumerate(frames):
            if f is None:
                fs.append(None)
                continue
            te = f.T if tend is None else min(f.T, tend)
            S_top = P_part[k] if (tend is not None and f.T > tend) else 0
            b = block_part(f.dec, ts, te, BL, nlanes, S_top, warm)
            if warm == 90:
                b30 = block_part(f.dec, ts, te, BL, nlanes, S_top, 30)
                w.fixed90 += int((b["fixed"] & ~b30["fixed"]).sum())
            fs.append(b)
        warm_here, depth = warm, [0] * len(frames)
        for ps in range(17 if not lat else 65):
            chs = [block_pass(f.dec, b) if b is not None else None for f, b in zip(frames, fs)]
            n = sum(int(c.sum()) for c in chs if c is not None)
            if ps == 0:
                w.miss0[pi] = n
                w.frame_miss0[pi] = [np.flatnonzero(c) if c is not None else np.zeros(0, np.int64) for c in chs]
                if warm_here == 90:
                    w.still_miss_90 += n
            if n == 0:
                break
            if ps == 0 and warm == 30 and n >= HARD_MISSES and not lat:
                warm = 90
                w.warm_switch.append(pi)
                w.c[7] += 1
            for k, (f, b, c) in enumerate(zip(frames, fs, chs)):
                if c is not None and c.any():
                    block_retrace(f.dec, b, c)
                    depth[k] += 1
        else:
            raise AssertionError("general form: pass bound reached")
        w.passes[pi], w.depth[pi] = ps, depth
        for k, (f, b) in enumerate(zip(frames, fs)):
            if b is not None:
                block_bits(b, w.bits[k])
                P_part[k] = int(b["P_out"][0])
    return w


def is_fast(frames):
    return all(f is not None for f in frames) and len({f.fb for f in frames}) == 1 and frames[0].fb % 16 == 0


def packed_wave(frames, long_launch):
    """the packed kernels' wave of four frame slots: long_launch = the launch's longest frame exceeds one segment"""
    if is_fast(frames):
        return fast_wave_long(frames) if long_launch else fast_wave_short(frames)
    return general_wave(frames)


def lat_wave(frame):
    return general_wave([frame], nlanes=64, lat=True)


# ---- generators: seeded, numpy only ------------------------------------------------------------------------------------
def xs_bytes(seed, n, lanes=256):
    """n bytes from `lanes` xorshift64 streams (13, 7, 17; byte = (x >> 11) & 255, as tests/reffix.py) advanced together"""
    s = (np.arange(1, lanes + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed & M64)) | _ONE
    a, b, c, d = np.uint64(13), np.uint64(7), np.uint64(17), np.uint64(11)
    steps = (n + lanes - 1) // lanes + 4
    out = np.empty((steps, lanes), np.uint8)
    for i in range(steps):
        s ^= s << a
        s ^= s >> b
        s ^= s << c
        out[i] = (s >> d).astype(np.uint8)
    return out[4:].reshape(-1)[:n]


_POLYS = (109, 79, 83, 109)
# amplitude of a hard symbol around 128 for Eb/N0 = 8, 3, 2 dB at rate 1/4 with a noise sigma of 32 (32 * sqrt(2 Es/N0))
AMP = {None: 127, 8: 57, 3: 32, 2: 28}


def encode(bits):
    """mother code, numpy: four hard symbols 0/1 per step, six zero tail bits appended"""
    b = np.concatenate([np.zeros(7, np.uint8), np.asarray(bits, np.uint8), np.zeros(TAIL, np.uint8)])
    n = b.size - 7
    out = np.zeros((n, 4), np.uint8)
    for j, poly in enumerate(_POLYS):
        for k in range(8):
            if (poly >> k) & 1:
                out[:, j] ^= b[7 - k:7 - k + n]
    return out.reshape(-1)


def base_symbols(fb, seed, db):
    """random bits through the mother code; db None: noise-free 1/255, else +-AMP[db] around 128 plus integer noise of
    sigma 32 (the sum of four uniform bytes, scaled: no floating point, the same bytes everywhere)"""
    n = 4 * (fb + TAIL)
    r = xs_bytes(seed, fb + 4 * n)
    hard = encode(r[:fb] >> 7).astype(np.int64)
    if db is None:
        return np.where(hard, 255, 1).astype(np.uint8)
    if db == "hf":  # hard decisions 0/255, about one symbol in six inverted: metrics reach 150 exactly, the comparators differ
        return np.where(hard ^ (r[fb:fb + n] < 40), 255, 0).astype(np.uint8)
    noise = ((r[fb:].reshape(4, n).astype(np.int64).sum(axis=0) - 510) * 111) >> 9
    return np.clip(128 + (2 * hard - 1) * AMP[db] + noise, 0, 255).astype(np.uint8)


BURSTS = ("erasure", "near", "uniform", "hard")


def add_burst(sym, kind, end_step, length, seed, a=2):
    """overwrite the symbols of steps [end_step - length, end_step) (clipped to the frame)"""
    sym = sym.copy()
    lo, hi = max(end_step - length, 0) * 4, min(end_step * 4, sym.size)
    if hi <= lo:
        return sym
    r = xs_bytes(seed ^ 0x5DEECE66D, hi - lo)
    if kind == "erasure":
        sym[lo:hi] = 128
    elif kind == "near":
        sym[lo:hi] = 128 - a + r % (2 * a + 1)
    elif kind == "uniform":
        sym[lo:hi] = r
    elif kind == "hard":
        sym[lo:hi] = (r >> 7) * 255
    else:
        raise ValueError(kind)
    return sym


class Spec:
    """a directed frame's recipe: reproducible from these numbers alone"""

    def __init__(self, fb, seed, db, bursts=()):
        self.fb, self.seed, self.db, self.bursts = fb, seed, db, tuple(bursts)

    def key(self):
        return (self.fb, self.seed, self.db, self.bursts)

    def symbols(self):
        sym = base_symbols(self.fb, self.seed, self.db)
        for i, (kind, end, length) in enumerate(self.bursts):
            sym = add_burst(sym, kind, end, length, self.seed * 31 + i)
        return sym


_frames = {}


def make_frame(O, spec, ge=False):
    key = (spec.key(), ge)
    if key not in _frames:
        sym = spec.symbols()
        _frames[key] = Frame(spec.fb, sym, O.decisions(spec.fb, sym, ge=ge), tag=repr(spec.key()))
    return _frames[key]


# ---- waves, classes, the search ------------------------------------------------------------------------------------------
def clean_spec(fb, k=0):
    """a noise-free frame of random bits: company that never fails a check or makes a wave give up (asserted by the host test)"""
    return Spec(fb, 1000 + k, None)


class Wave:
    """four frame slots (Spec or None) and the launch they sit in: entry "uniform" (one framebits) or "desc" (a descriptor
    table of fewer than 16 frames: not sorted, waves as listed); long_launch: the launch's longest frame exceeds one segment"""

    def __init__(self, specs, entry, long_launch, directed=0):
        self.specs, self.entry, self.long_launch, self.directed = list(specs), entry, long_launch, directed

    def frames(self, O, ge=False):
        return [make_frame(O, s, ge) if s is not None else None for s in self.specs]

    def model(self, O, ge=False):
        return packed_wave(self.frames(O, ge), self.long_launch)

    def to_json(self):
        return dict(specs=[None if s is None else [s.fb, s.seed, s.db, [list(b) for b in s.bursts]] for s in self.specs],
                    entry=self.entry, long=self.long_launch, directed=self.directed)

    @staticmethod
    def from_json(d):
        specs = [None if s is None else Spec(s[0], s[1], s[2], [tuple(b) for b in s[3]]) for s in d["specs"]]
        return Wave(specs, d["entry"], d["long"], d["directed"])


def _runs(parts):
    """lengths of the runs of consecutive part numbers"""
    out, n = [], 0
    for i, p in enumerate(parts):
        n = n + 1 if i and p == parts[i - 1] + 1 else 1
        if i + 1 == len(parts) or parts[i + 1] != p + 1:
            out.append(n)
    return out


def _only_frame(w, part, k):
    fm = w.frame_miss0.get(part)
    return fm is not None and fm[k].size > 0 and all(m.size == 0 for j, m in enumerate(fm) if j != k)


def fast_classes(wave, w):
    """classes of a fast-form trace (single-segment kernel, or the long-frame kernel's parts after the forward pass)"""
    out = set()
    fb = wave.specs[0].fb
    T = fb + TAIL
    for p, fm in w.frame_miss0.items():
        hi = T - 256 * p
        lo = hi - 256 if hi > 256 + TAIL else TAIL
        nl = (hi - lo) >> 4
        n = sum(m.size for m in fm)
        for k, m in enumerate(fm):
            if n == 1 and m.size == 1 and nl == 16:
                out.add("fast.one_miss.lane%d" % m[0])
            if m.size and _only_frame(w, p, k):
                out.add("fast.miss_in_slot%d" % k)
            if m.size and nl < 16 and lo == TAIL:
                out.add("fast.miss_in_short_lowest_part")
            if m.size and nl >= 3 and (nl - 3) in m:
                out.add("fast.miss_first_lane_below_top")
        for d in w.depth[p]:
            if d:
                out.add("fast.cascade%d" % min(d, 11))
        if nl <= 3:
            out.add("fast.nl%d" % nl)
    return out


def inflight_classes(wave, w):
    out = set()
    fb = wave.specs[0].fb
    NP = (fb + 255) >> 8
    failed = [p for p, was in w.chain if was]
    short_bottom = fb % 256 != 0
    for p in failed:
        if p == 1:
            out.add("inflight.fail_p1")
        if p == NP - 1 and NP > 2:
            out.add("inflight.fail_bottom_short" if short_bottom else "inflight.fail_bottom_full")
        if 1 < p < NP - 1:
            out.add("inflight.fail_middle")
    for (p, was), who in zip(w.chain, w.chain_frames):
        if was and len(who) == 1:  # the one frame whose top position was wrong
            out.add("inflight.fail_in_slot%d" % who[0])
    runs = _runs(sorted(failed))
    if len(runs) >= 2:
        out.add("inflight.two_nonadjacent")
    if w.gave_up_at is None:
        for r in runs:
            out.add("inflight.adjacent_run%d" % min(r, 4))
    if w.first_ok:
        out.add("inflight.first_ok_then_fail")
    for p, (n, per) in w.inflight_miss.items():
        if p >= 2 and n == 7:
            out.add("inflight.total7_keeps_tracing:" + "+".join(str(x) for x in per if x))
        if p >= 2 and n == 8:
            out.add("inflight.total8_gives_up:" + "+".join(str(x) for x in per if x))
        if p == 1 and n >= HARD_MISSES:
            out.add("inflight.hard_at_part1")
    g = w.gave_up_at
    if g is not None:
        good = (NP - 1) - g  # in-flight parts traced before the one that gave up
        out.add("inflight.giveup_first" if good == 0 else "inflight.giveup_after%s" % (good if good <= 2 else "5plus" if good >= 5 else "3to4"))
        if failed:
            out.add("inflight.failed_checked_below_unchecked")
    if NP == 2:
        out.add("inflight.NP2")
    if NP == 36:
        out.add("inflight.NP36")
    return out | fast_classes(wave, w)


def general_classes(wave, w):
    out = set()
    fbs = [s.fb for s in wave.specs if s is not None]
    d = wave.specs[wave.directed].fb
    busy = sum(w.miss0.values()) > 0
    if not busy:
        return out
    if len(set(fbs)) == 4:
        out.add("general.four_lengths")
    if d % 16:
        out.add("general.not_multiple_of_16")
    if d == max(fbs) and fbs.count(d) == 1:
        out.add("general.directed_longest")
    if d == min(fbs) and fbs.count(d) == 1:
        out.add("general.directed_shortest")
    if 0 in w.warm_switch and len(w.miss0) > 1:
        out.add("general.hard_first_part")
    if w.still_miss_90:
        out.add("general.miss_at_90")
    if w.fixed90:
        out.add("general.fixed_under_90_only")
    if max(max(x) for x in w.depth.values()) >= 6:
        out.add("general.cascade6plus")
    out.add("general.long_kernel" if wave.long_launch else "general.single_segment")
    return out


def lat_classes(spec, w):
    out = set()
    BL = 6 * ((spec.fb + 383) // 384)
    m = w.frame_miss0[0][0]
    if not m.size:
        return out
    if BL in (6, 12, 144):
        out.add("lat.BL%d" % BL)
    if 0 in m:
        out.add("lat.miss_lane0")
    T = spec.fb + TAIL
    q = np.arange(64)
    spec_lanes = q[(TAIL + q * BL < T) & (T - 1 - (TAIL + q * BL) > BL - 1 + 30)]
    if spec_lanes.size and spec_lanes[-1] in m:
        out.add("lat.miss_top_speculative_lane")
    out.add("lat.cascade%d" % w.depth[0][0])
    return out


def wave_classes(O, wave):
    w = wave.model(O)
    if w.form == "fast":
        return fast_classes(wave, w), w
    if w.form == "inflight":
        return inflight_classes(wave, w), w
    return general_classes(wave, w), w


# what the directed set must populate with at least NEED distinct directed frames each (the one_miss lanes and the cascade depths
# count together as one class each in the issue's list; here every lane and every depth is required on its own, with one frame)
NEED = 3
CLASSES = (
    ["fast.one_miss.lane%d" % q for q in range(14)] + ["fast.miss_in_slot%d" % k for k in range(4)] +
    ["fast.miss_in_short_lowest_part", "fast.nl1", "fast.nl2", "fast.nl3", "fast.miss_first_lane_below_top"] +
    ["fast.cascade%d" % d for d in range(1, 11)] +
    ["inflight.fail_p1", "inflight.fail_bottom_short", "inflight.fail_bottom_full", "inflight.fail_middle"] +
    ["inflight.fail_in_slot%d" % k for k in range(4)] +
    ["inflight.two_nonadjacent"] + ["inflight.adjacent_run%d" % r for r in (1, 2, 3, 4)] +
    ["inflight.first_ok_then_fail", "inflight.total7_keeps_tracing", "inflight.total8_gives_up", "inflight.giveup_first",
     "inflight.giveup_after1", "inflight.giveup_after2", "inflight.giveup_after5plus", "inflight.hard_at_part1",
     "inflight.failed_checked_below_unchecked", "inflight.NP2", "inflight.NP36"] +
    ["general.four_lengths", "general.not_multiple_of_16", "general.directed_longest", "general.directed_shortest",
     "general.hard_first_part", "general.miss_at_90", "general.fixed_under_90_only", "general.cascade6plus",
     "general.single_segment", "general.long_kernel"] +
    ["lat.BL6", "lat.BL12", "lat.BL144", "lat.miss_lane0", "lat.miss_top_speculative_lane"] +
    # frames with misses whose output differs between the `> 150` and the `>= 150` renormalisation (hard-decision base)
    ["cmp.fast", "cmp.inflight", "cmp.general"])
ONE_EACH = tuple(c for c in CLASSES if c.startswith("fast.one_miss.lane") or c.startswith("fast.cascade"))
REQUIRED = tuple(["fast.cascade%d" % d for d in range(1, 11)] +
                 ["inflight.first_ok_then_fail", "inflight.total7_keeps_tracing", "inflight.total8_gives_up",
                  "inflight.giveup_after1", "inflight.giveup_after2", "inflight.giveup_after5plus"])
# classes the generator did not reach: (class, reason).  At most three, none of REQUIRED.
NOT_REACHED = ()


def _h(i, salt):
    x = ((i + 1) * 0x9E3779B97F4A7C15 + salt * 0xD1B54A32D192ED03) & M64
    x ^= x >> 29
    x = (x * 0xBF58476D1CE4E5B9) & M64
    return x ^ (x >> 32)


def _pick(i, salt, seq):
    return seq[_h(i, salt) % len(seq)]


def candidate(family, i):
    """the i-th candidate wave of a family: every choice is a hash of i"""
    kind = _pick(i, 1, BURSTS)
    db = _pick(i, 2, (None, 8, 8, 3, 3, 2))
    seed = 1 + _h(i, 3) % 100000
    slot = _h(i, 4) % 4
    if family == "fast":
        fb = _pick(i, 5, (768, 768, 768, 400, 704, 272, 288, 304, 16, 32, 48))
        T = fb + TAIL
        length = _pick(i, 6, (34, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160, 176, 192, 208, 224, 240, 256))
        end = TAIL + 16 * (_h(i, 7) % ((T - TAIL) // 16 + 1)) + _pick(i, 8, (0, 0, 3, 8, 13, 30, 45))
        sp = Spec(fb, seed, db, [(kind, min(end, T), length)])
        specs = [clean_spec(fb, k) for k in range(4)]
        specs[slot] = sp
        return Wave(specs, "uniform", False, slot)
    if family == "inflight":
        fb = _pick(i, 5, (3072, 3072, 3072, 3200, 1024, 3088, 6912))
        T, NP = fb + TAIL, (fb + 255) >> 8
        p = _pick(i, 9, (1, 1, 2, NP // 2, NP - 2, NP - 1, NP - 1, 1 + _h(i, 10) % (NP - 1)))
        hi = T - 256 * p
        length = _pick(i, 6, (20, 30, 36, 40, 44, 48, 56, 64, 80, 100, 140, 200, 300, 400, 600))
        end = hi + _pick(i, 8, (-200, -120, -60, -20, 0, 10, 20, 30, 40, 60, 100, 200))
        bursts = [(kind, max(min(end, T), 8), length)]
        if _h(i, 11) % 4 == 0:  # a second burst some parts away
            p2 = 1 + _h(i, 12) % (NP - 1)
            bursts.append((_pick(i, 13, BURSTS), max(T - 256 * p2 + _pick(i, 14, (0, 20, 40)), 8), _pick(i, 15, (30, 40, 60, 100, 300))))
        sp = Spec(fb, seed, db, bursts)
        specs = [clean_spec(fb, k) for k in range(4)]
        specs[slot] = sp
        return Wave(specs, "uniform", True, slot)
    if family == "comb":  # one short burst at the top of each of r consecutive parts: a run of failing parts, no give-up
        fb = _pick(i, 5, (3072, 3200, 6912))
        T, NP = fb + TAIL, (fb + 255) >> 8
        r = 4 + _h(i, 6) % 3
        p0 = 1 + _h(i, 7) % (NP - r)
        off, length = _pick(i, 8, (16, 24, 30)), _pick(i, 9, (30, 36, 40, 44))
        sp = Spec(fb, seed, db, [(kind, T - 256 * (p0 + j) + off, length) for j in range(r)])
        specs = [clean_spec(fb, k) for k in range(4)]
        specs[slot] = sp
        return Wave(specs, "uniform", True, slot)
    if family == "long_burst":  # 300 .. 600 dead steps: parts that agree with the part above on the same wrong survivor
        fb = _pick(i, 5, (3072, 3072, 6912))
        T = fb + TAIL
        length = _pick(i, 6, (300, 400, 500, 600))
        sp = Spec(fb, seed, _pick(i, 2, (8, 8, 3)), [(_pick(i, 1, ("erasure", "erasure", "near", "uniform")), min(T, 300 + _h(i, 7) % T), length)])
        specs = [clean_spec(fb, k) for k in range(4)]
        specs[slot] = sp
        return Wave(specs, "uniform", True, slot)
    if family == "general":
        fb = _pick(i, 5, (778, 500, 302, 770, 1000, 3070, 2002, 6910, 1234))
        T = fb + TAIL
        length = _pick(i, 6, (40, 60, 100, 150, 200, 300, 400, 600))
        end = min(T, 8 + _h(i, 7) % T + length // 2) if _h(i, 16) % 3 else T
        sp = Spec(fb, seed, db, [(kind, max(end, 8), length)])
        mode = _h(i, 17) % 3
        if mode == 0:  # the longest of four different lengths
            others = [max(fb - 2 * (37 + 61 * k), 2) for k in range(3)]
        elif mode == 1:  # the shortest
            others = [fb + 2 * (5 + 33 * k) for k in range(3)]
        else:  # equal lengths that are no multiple of 16, or one empty slot
            others = [fb, fb, fb] if fb % 16 else [fb, fb, 0]
        specs, j = [], 0
        for k in range(4):
            if k == slot:
                specs.append(sp)
            else:
                specs.append(clean_spec(others[j], k) if others[j] else None)
                j += 1
        if specs[3] is None or specs.count(None):  # an empty slot is the batch's tail: it must come last
            specs = [s for s in specs if s is not None] + [None] * specs.count(None)
            slot = specs.index(sp)
        return Wave(specs, "desc", max(s.fb for s in specs if s is not None) > SHORT_MAX, slot)
    raise ValueError(family)


def lat_candidate(i):
    kind = _pick(i, 1, BURSTS)
    db = _pick(i, 2, (None, 8, 3, 2))
    fb = _pick(i, 5, (384, 200, 768, 400, 9216, 8834, 3072))
    T = fb + TAIL
    BL = 6 * ((fb + 383) // 384)
    length = _pick(i, 6, (40, 60, 100, 200, 400)) * (1 if BL < 100 else 4)
    where = _h(i, 7) % 4
    end = (TAIL + BL + 35 if where == 0 else T - 20 if where == 1 else 8 + _h(i, 8) % T)
    return Spec(fb, 1 + _h(i, 3) % 100000, db, [(kind, max(min(end, T), 8), length)])


def compose_totals(O, pool_fb=3072, part=5, limit=4000):
    """waves whose in-flight pass-0 misses at one part total exactly 7 and exactly 8, spread over the four frames in
    different ways: frames with 1 .. 8 misses at that part (and none elsewhere) are searched, then combined"""
    T = pool_fb + TAIL
    hi = T - 256 * part
    by = {}
    for i in range(limit):
        length = _pick(i, 21, (24, 30, 36, 40, 48, 56, 64, 72, 80, 96, 112, 128, 144, 160, 176))
        end = hi - 16 * (_h(i, 22) % 8) + _pick(i, 23, (0, 5, 11, 20, 30))
        sp = Spec(pool_fb, 1 + _h(i, 24) % 100000, _pick(i, 25, (None, 8, 8, 3)), [(_pick(i, 26, BURSTS), end, length)])
        f = make_frame(O, sp)
        trs = {p: f.fast(p, 0, spec=True) for p in (part - 1, part, part + 1)}
        n = {p: (t.miss[0].size if t.miss else 0) for p, t in trs.items()}
        if 1 <= n[part] <= 8 and n[part - 1] == 0 and n[part + 1] == 0 and len(by.setdefault(n[part], [])) < 3:
            by[n[part]].append(sp)
        if all(len(by.get(m, ())) >= 2 for m in (1, 2, 3, 4, 7, 8)):
            break
    waves = []
    for combo in ((7,), (3, 4), (1, 2, 4), (8,), (4, 4), (1, 3, 4), (2, 2, 4)):
        used, specs = {}, []
        for m in combo:
            k = used.get(m, 0)
            if k >= len(by.get(m, ())):
                specs = None
                break
            specs.append(by[m][k])
            used[m] = k + 1
        if specs is None:
            continue
        for rot in range(2):
            full = specs + [clean_spec(pool_fb, k) for k in range(4 - len(specs))]
            full = full[rot:] + full[:rot]
            waves.append(Wave(full, "uniform", True, full.index(specs[0])))
    return waves


def search(O, verbose=False, limits=(("fast", 1500), ("inflight", 2500), ("comb", 300), ("long_burst", 1500), ("general", 800))):
    """-> the directed set: waves kept because they add a member to a class that still needs one"""
    have, kept, lat = {c: set() for c in CLASSES}, [], []

    def need(c):
        base = c.split(":")[0]
        return base in have and len(have[base]) < (1 if base in ONE_EACH else NEED)

    def offer(wave, classes):
        new = [c for c in classes if need(c)]
        if not new:
            return False
        key = wave.specs[wave.directed].key()
        for c in classes:
            if c.split(":")[0] in have:
                have[c.split(":")[0]].add(key + ((c.split(":")[1],) if ":" in c else ()))
        return True

    for wave in compose_totals(O) + [
            Wave([Spec(9216, 77, 3, [("erasure", 4000, 60)])] + [clean_spec(9216, k) for k in (1, 2, 3)], "uniform", True, 0),
            Wave([Spec(9216, 78, 8, [("uniform", 9000, 300)])] + [clean_spec(9216, k) for k in (1, 2, 3)], "uniform", True, 0),
            Wave([Spec(9216, 79, 2, [("hard", 300, 80)])] + [clean_spec(9216, k) for k in (1, 2, 3)], "uniform", True, 0)]:
        if offer(wave, wave_classes(O, wave)[0]):
            kept.append(wave)
    for i in range(60):  # NP = 2: four 512-bit frames behind a long wave in one descriptor table
        sp = Spec(512, 1 + _h(i, 31) % 100000, _pick(i, 32, (8, 3)), [(_pick(i, 33, BURSTS), 262 + _pick(i, 34, (0, 10, 20, 30, 40)), _pick(i, 35, (30, 40, 60, 100)))])
        wave = Wave([clean_spec(512, 0), sp, clean_spec(512, 2), clean_spec(512, 3)], "desc", True, 1)
        if offer(wave, wave_classes(O, wave)[0]):
            kept.append(wave)
    for family, limit in limits:
        for i in range(limit):
            fam = "inflight" if family in ("comb", "long_burst") else family
            if not any(need(c) for c in CLASSES if c.startswith(fam) or (family == "inflight" and c.startswith("fast"))):
                break
            wave = candidate(family, i)
            if offer(wave, wave_classes(O, wave)[0]):
                kept.append(wave)
                if verbose:
                    print(family, i, len(kept), flush=True)
    for i in range(400):  # the comparator family: a hard-decision base, kept where the two comparators decode differently
        if not any(need(c) for c in CLASSES if c.startswith("cmp")):
            break
        wave = candidate(("fast", "inflight", "general")[i % 3], 100000 + i)
        d = wave.directed
        sp = Spec(wave.specs[d].fb, wave.specs[d].seed, "hf", wave.specs[d].bursts)
        wave.specs[d] = sp
        sym = sp.symbols()
        if np.array_equal(O.decode_batch(sp.fb, sym), O.decode_batch(sp.fb, sym, ge=True)):
            continue
        w = wave.model(O)
        if sum(w.miss0.values()) + sum(n for n, _ in w.inflight_miss.values()) and offer(wave, {"cmp." + w.form}):
            kept.append(wave)
    depth = 0
    for i in range(600):
        sp = lat_candidate(i)
        w = lat_wave(make_frame(O, sp))
        cl = lat_classes(sp, w)
        d = w.depth[0][0]
        new = [c for c in cl if need(c)] or (d > depth)
        if new:
            depth = max(depth, d)
            for c in cl:
                if c in have:
                    have[c].add(sp.key())
            lat.append(sp)
        if not any(need(c) for c in CLASSES if c.startswith("lat")) and i >= 200:
            break
    return kept, lat, have


# ---- the committed directed set and the batches the GPU tests launch -----------------------------------------------------
DIRECTED_JSON = os.path.join(GOLD, "tb_directed.json")  # what search() kept: recipes (numbers), regenerated by `python tests/tbdirect.py`


def save_directed(kept, lat, path=DIRECTED_JSON):
    import json
    with open(path, "w") as f:
        json.dump(dict(waves=[w.to_json() for w in kept], lat=[[s.fb, s.seed, s.db, [list(b) for b in s.bursts]] for s in lat]),
                  f, separators=(",", ":"))
        f.write("\n")


_directed = None


def load_directed():
    """-> (waves, latency-kernel frames) of the committed set"""
    global _directed
    if _directed is None:
        import json
        with open(DIRECTED_JSON) as f:
            d = json.load(f)
        _directed = ([Wave.from_json(w) for w in d["waves"]],
                     [Spec(s[0], s[1], s[2], [tuple(b) for b in s[3]]) for s in d["lat"]])
    return _directed


def pinned_specs():
    """every distinct frame of the directed set (companions included), in order of first appearance, then the latency frames"""
    waves, lat = load_directed()
    seen, out = set(), []
    for sp in [s for w in waves for s in w.specs if s is not None] + list(lat):
        if sp.key() not in seen:
            seen.add(sp.key())
            out.append(sp)
    return out


PIN_COLS = ("framebits", "in_fnv", "out_gt", "out_ge")  # columns of reference_tb_paths.npy (uint64), one row per pinned_specs()


def pinned_rows(decode, fnv_rows):
    """decode(fb, sym, ge) -> the output bytes of one frame; fnv_rows: reffix.fnv1a64_rows"""
    specs = pinned_specs()
    syms = [s.symbols() for s in specs]
    rows = np.zeros((len(specs), len(PIN_COLS)), np.uint64)
    rows[:, 0] = [s.fb for s in specs]
    rows[:, 1] = fnv_rows(syms)
    rows[:, 2] = fnv_rows([decode(s.fb, x, False) for s, x in zip(specs, syms)])
    rows[:, 3] = fnv_rows([decode(s.fb, x, True) for s, x in zip(specs, syms)])
    return rows


def census(O):
    """the committed set through the models (comparator `>`): class -> distinct directed frames, and the deepest re-trace
    cascades per form; every model's bits are compared with the serial chainback on the way"""
    waves, lat = load_directed()
    have = {c: set() for c in CLASSES}
    deepest = {"fast": 0, "general": 0, "lat": 0}
    for wave in waves:
        cl, w = wave_classes(O, wave)
        for k, f in enumerate(wave.frames(O)):
            assert f is None or np.array_equal(w.bits[k], f.true()[0]), ("model differs from ChainBack", w.form, wave.specs[k].key())
        sp = wave.specs[wave.directed]
        if sp.db == "hf":
            sym = sp.symbols()
            if (sum(w.miss0.values()) + sum(n for n, _ in w.inflight_miss.values())
                    and not np.array_equal(O.decode_batch(sp.fb, sym), O.decode_batch(sp.fb, sym, ge=True))):
                cl = cl | {"cmp." + w.form}
        for c in cl:
            base = c.split(":")[0]
            if base in have:
                have[base].add(sp.key() + ((c.split(":")[1],) if ":" in c else ()))
        form = "general" if w.form == "general" else "fast"
        deepest[form] = max([deepest[form]] + [max(d) for d in w.depth.values()])
    for sp in lat:
        f = make_frame(O, sp)
        w = lat_wave(f)
        assert np.array_equal(w.bits[0], f.true()[0]), ("latency model differs from ChainBack", sp.key())
        for c in lat_classes(sp, w):
            if c in have:
                have[c].add(sp.key())
        deepest["lat"] = max(deepest["lat"], w.depth[0][0])
    return have, deepest


class Batch:
    """one launch: waves of four slots; uniform entry (framebits) or a descriptor table of fewer than 16 frames"""

    def __init__(self, name, waves, framebits=None):
        self.name, self.waves, self.framebits = name, waves, framebits
        self.specs = [s for w in waves for s in w.specs if s is not None]
        assert all(None not in w.specs for w in waves[:-1]), "an empty slot is the tail of the batch"
        assert framebits is not None or len(self.specs) < 16, "a longer table is sorted on the device: waves would regroup"
        self.long_launch = max(s.fb for s in self.specs) > SHORT_MAX
        assert all(w.long_launch == self.long_launch for w in waves), name

    def lengths(self):
        return [s.fb for s in self.specs]

    def symbols(self):
        """list of the frames' symbol arrays"""
        return [s.symbols() for s in self.specs]

    def counters(self, O, ge=False):
        """the eight -DVIT_DIAG_SPEC counters the packed kernel adds for this launch"""
        return sum((w.model(O, ge).c for w in self.waves), np.zeros(8, np.int64))


def batches(waves):
    """the directed waves as launches: one uniform launch per framebits, descriptor tables of at most three waves"""
    out, by_fb = [], {}
    for w in waves:
        if w.entry == "uniform":
            by_fb.setdefault(w.specs[0].fb, []).append(w)
    for fb in sorted(by_fb):
        out.append(Batch("uniform%d" % fb, by_fb[fb], fb))
    for flag in (False, True):
        cur = []
        for w in [w for w in waves if w.entry == "desc" and w.long_launch == flag]:
            if flag and max(s.fb for s in w.specs if s is not None) <= SHORT_MAX and not cur:
                # short frames take the long-frame kernel only in a launch that has a long frame: a clean long wave leads
                cur.append(Wave([clean_spec(800, k) for k in range(4)], "desc", True, 0))
            cur.append(w)
            if len(cur) == 3 or None in w.specs:
                out.append(Batch("desc%s%d" % ("L" if flag else "S", len(out)), cur))
                cur = []
        if cur:
            out.append(Batch("desc%s%d" % ("L" if flag else "S", len(out)), cur))
    return out


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(GOLD[:-len("/golden")]))
    import _vitpkg
    O_ = _vitpkg.load_oracle()
    O_.build()
    kept_, lat_, have_ = search(O_, verbose=True)
    save_directed(kept_, lat_)
    for c_ in CLASSES:
        print("%-44s %d" % (c_, len(have_[c_])))
