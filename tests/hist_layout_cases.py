"""Frames directed at the decision-history layout of the packed kernels (csrc/vit_pk.hip: acs_step), and the launches of
tests/test_gpu_hist_layout.py, kept apart from pytest so that the 768-bit launches can run once more in a child process on
libviterbi_general.so (-DVIT_FIC_FIXED=0).

acs_step drops a step's decision into the history word with one v_bfi from the packed difference m0 - m1 (m2 - m3), at a bit
position 8..15 of its 16-bit half: that is right only as long as bits 8..15 of the difference are all copies of its sign, i.e.
|difference| <= 255, and the positions are right only if the block's one `>> 8` sits between steps 7 and 8 (after step 5 in a
six-step last block).  So the layout can go wrong only on differences of a large magnitude and at the shift points.  The frames
here are kept because a numpy add-compare-select (the trellis of deconvolve.cpp restated, checked against the oracle's
decision words) says they contain differences of BOTH signs with bit 7 != bit 8 of their 16-bit two's complement (d >= 128,
d <= -129), for m0 - m1 and for m2 - m3, at block-relative steps 0, 7, 8 and 15 and in the six-step last block.

What a length can reach, from the trellis and not from any decoder: the metrics start at 63 (state 0 at 0), so at step 0
|d| <= 63 + 63 < 128 - "block-relative step 0" needs a second block.  fb = 2 (T = 8, one short block) has steps 0..7 only:
position 7.  fb = 10 (T = 16): positions 7, 8, 15.  From fb = 26 (T = 32) on: all four.  The last block has six steps where
T = 6 mod 16 (768, 784).

Inputs are seeded streams of tests/reffix.py (xorshift_bytes) shaped like the existing families: hard decisions (bit 7 of the
stream -> 0 / 255, the reference fixtures' hard family) and the saturation stress of tests/test_gpu_parity.py (constant 0,
constant 255, runs of 64 equal bytes).

As a script: runs the 768-bit launches on the library in VITERBI_AMD_LIB, prints one line per launch group, exit status 0 only if
all agree.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import reffix  # noqa: E402

TAIL = 6
GUARD, SENTINEL = 64, 0xA5
FRAMEBITS = (2, 10, 26, 762, 768, 784)  # T = 8: one short block; 16: one full block; 32; general / fixed / long-frame kernel
POSITIONS = (0, 7, 8, 15)
DESC_CHUNK = 12  # a descriptor table of fewer than 16 frames is consumed as listed: the waves stay as built


def ncandidates(fb):
    """candidates per family: a short frame has few steps to reach a large difference at a given one, and costs little"""
    return 512 if fb <= 26 else 48


def reachable_positions(fb):
    """block-relative steps at which |d| >= 128 is possible at all for this length (see the module docstring)"""
    T = fb + TAIL
    return tuple(p for p in POSITIONS if any(t % 16 == p for t in range(1, T)))


def has_last6(fb):
    return (fb + TAIL) % 16 == 6


# ---- the trellis in numpy, over many frames at once ----------------------------------------------------------------------
def _masks():
    i = np.arange(32)
    par = lambda x: np.array([bin(int(v)).count("1") & 1 for v in x])  # noqa: E731
    return np.stack([par((2 * i) & p) * 255 for p in (109, 79, 83, 109)]).astype(np.int64)


def acs(sym, ge=False):
    """sym: (n, 4 T) uint8 -> (d01, d23, dec): the differences m0 - m1 and m2 - m3 of every butterfly (n, T, 32) int16 as the
    kernel forms them (after the 255 clamp), and the decision words (n, T) uint64 as ChainBack reads them"""
    sym = np.asarray(sym, np.int64)
    n, T = sym.shape[0], sym.shape[1] // 4
    sym = sym.reshape(n, T, 4)
    mask = _masks()
    avg = lambda a, b: (a + b + 1) >> 1  # noqa: E731
    old = np.full((n, 64), 63, np.int64)
    old[:, 0] = 0
    d01, d23 = np.empty((n, T, 32), np.int16), np.empty((n, T, 32), np.int16)
    dec = np.zeros((n, T), np.uint64)
    sh0, sh1 = (2 * np.arange(32)).astype(np.uint64), (2 * np.arange(32) + 1).astype(np.uint64)
    for t in range(T):
        x = sym[:, t, :, None] ^ mask[None]
        metric = avg(avg(x[:, 0], x[:, 1]), avg(x[:, 2], x[:, 3])) >> 2
        mm = 63 - metric
        m0, m1 = np.minimum(old[:, :32] + metric, 255), np.minimum(old[:, 32:] + mm, 255)
        m2, m3 = np.minimum(old[:, :32] + mm, 255), np.minimum(old[:, 32:] + metric, 255)
        d01[:, t], d23[:, t] = m0 - m1, m2 - m3
        k0, k1 = m1 <= m0, m3 <= m2
        new = np.empty((n, 64), np.int64)
        new[:, 0::2], new[:, 1::2] = np.where(k0, m1, m0), np.where(k1, m3, m2)
        dec[:, t] = np.bitwise_or.reduce((k0.astype(np.uint64) << sh0) | (k1.astype(np.uint64) << sh1), axis=1)
        if t & 1:
            hit = (new[:, 0] >= 150) if ge else (new[:, 0] > 150)
            new = np.where(hit[:, None], np.maximum(new - 63, 0), new)
        old = new
    return d01, d23, dec


# ---- candidates and the directed set -------------------------------------------------------------------------------------
def candidates(fb):
    """-> (n, 4 T) uint8: ncandidates(fb) frames each of the hard-decision family and of the saturation-stress family"""
    sl, CANDIDATES = reffix.sym_len(fb), ncandidates(fb)
    seeds = [((fb * 1000003 + k) * 0x9E3779B97F4A7C15 + 0x5851F42D4C957F2D) & reffix.M64 | 1 for k in range(2 * CANDIDATES)]
    rows = np.stack(reffix.xorshift_bytes(seeds, [sl] * len(seeds)))
    hard = ((rows[:CANDIDATES] >> 7) * 255).astype(np.uint8)
    stress = np.empty((CANDIDATES, sl), np.uint8)
    blk = rows[CANDIDATES:]
    stress[:] = np.repeat(blk[:, :sl // 64 + 1], 64, axis=1)[:, :sl]  # runs of 64 equal bytes
    stress[0], stress[1] = 0, 255
    stress[2::4] = np.repeat((blk[2::4, :sl // 64 + 1] >> 7) * 255, 64, axis=1)[:, :sl]  # runs of 64 symbols 0 / 255
    return np.concatenate([hard, stress])


def requirements(fb):
    """names of what the directed set of this length must contain"""
    where = ["step%d" % p for p in reachable_positions(fb)] + (["last6"] if has_last6(fb) else [])
    return ["%s.%s.%s" % (w, d, s) for w in where for d in ("d01", "d23") for s in ("pos", "neg")]


def coverage(fb, d01, d23):
    """-> (n, len(requirements)) bool and (n, len(requirements)) the largest magnitude that meets each requirement"""
    T = fb + TAIL
    t = np.arange(T)
    nb = (T + 15) >> 4
    sel = [(t % 16 == p) & (t >= 1) for p in reachable_positions(fb)] + ([t >= 16 * (nb - 1)] if has_last6(fb) else [])
    cov, mag = [], []
    for s in sel:
        for d in (d01, d23):
            x = d[:, s, :].reshape(d.shape[0], -1).astype(np.int64)
            # bit 7 != bit 8 of the 16-bit two's complement: 128 .. 255 and -255 .. -129
            p, q = np.where(x >= 128, x, 0).max(axis=1), np.where(x <= -129, -x, 0).max(axis=1)
            cov += [p > 0, q > 0]
            mag += [p, q]
    return np.stack(cov, axis=1), np.stack(mag, axis=1)


_directed = {}


def directed(fb):
    """-> (sym (k, 4 T), names of the requirements they meet, largest |d| among them): a greedy cover of requirements(fb) by
    the candidates (a frame is kept for what the trellis does under the `> 150` comparator)"""
    if fb not in _directed:
        cand = candidates(fb)
        d01, d23, _ = acs(cand)
        cov, mag = coverage(fb, d01, d23)
        names, need, keep = requirements(fb), np.ones(cov.shape[1], bool), []
        while need.any():
            gain = (cov & need).sum(axis=1)
            k = int(gain.argmax())
            if gain[k] == 0:
                break
            keep.append(k)
            need &= ~cov[k]
        met = [nm for nm, m in zip(names, ~need) if m]
        big = int(mag[keep].max()) if keep else 0
        _directed[fb] = (np.ascontiguousarray(cand[keep]), met, big)
    return _directed[fb]


def filler(fb):
    """the frame that fills the other three slots of a wave: uniform random bytes (the reference fixtures' soft family)"""
    return reffix.decoder_inputs([fb])[0][0]


def batch(fb):
    """every directed frame in each of the four slots of a wave, the other slots filled -> (16 k, 4 T) uint8"""
    sym = directed(fb)[0]
    out = np.tile(filler(fb), (16 * sym.shape[0], 1))
    for k in range(sym.shape[0]):
        for slot in range(4):
            out[16 * k + 4 * slot + slot] = sym[k]
    return out


# ---- the launches ---------------------------------------------------------------------------------------------------------
class Data:
    """batches and the oracle's bytes per comparator, computed once"""

    def __init__(self, O):
        self.O, self._sym, self._want = O, {}, {}

    def sym(self, fb):
        if fb not in self._sym:
            self._sym[fb] = batch(fb)
        return self._sym[fb]

    def want(self, fb, ge):
        if (fb, bool(ge)) not in self._want:
            self._want[fb, bool(ge)] = self.O.decode_batch(fb, self.sym(fb), nthreads=8, ge=bool(ge))
        return self._want[fb, bool(ge)]


def launch(V, torch, data, fb, ge, kernel, entry):
    """-> None or a message.  Output pre-filled with a sentinel, guard bytes on both sides, every byte compared."""
    sym, want = data.sym(fb), data.want(fb, ge)
    n, nb = sym.shape[0], (fb + 7) // 8
    d_sym = torch.from_numpy(sym).cuda()
    d_out = torch.full((n * nb + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    old, old_ge = V.set_kernel(kernel), V.set_renorm_ge(1 if ge else 0)
    try:
        if entry == "desc":
            for a in range(0, n, DESC_CHUNK):
                m = min(DESC_CHUNK, n - a)
                desc, sym_bytes, out_bytes = V.make_descs([fb] * m)
                assert sym_bytes == m * sym.shape[1] and out_bytes == m * nb
                V.decode_varlen_dev(d_sym[a:a + m].view(-1), d_out[GUARD + a * nb:], torch.from_numpy(desc.view(np.uint8)).cuda(), m, fb)
        else:
            V.decode_batch_dev(d_sym, d_out[GUARD:], fb, n)
        torch.cuda.synchronize()
    finally:
        V.set_renorm_ge(old_ge)
        V.set_kernel(old)
    got = d_out.cpu().numpy()
    if not ((got[:GUARD] == SENTINEL).all() and (got[GUARD + n * nb:] == SENTINEL).all()):
        return "wrote outside the output (fb=%d)" % fb
    bad = np.flatnonzero((got[GUARD:GUARD + n * nb].reshape(n, nb) != want).any(axis=1))
    if bad.size:
        return "fb=%d ge=%d kernel=%d %s: %d of %d frames differ from the oracle, first %s (directed frame, slot = %s)" % (
            fb, ge, kernel, entry, bad.size, n, bad[:6].tolist(), [(int(b) // 16, int(b) % 4) for b in bad[:6]])
    return None


KERNELS = (1, 2, 0)  # the one-frame-per-wave cross-check, the packed kernels, what the library picks itself
ENTRIES = ("uniform", "desc")


def case(V, torch, data, fb, ge):
    return [launch(V, torch, data, fb, ge, k, e) for k in KERNELS for e in ENTRIES]


def main():
    sys.path[:0] = [os.path.dirname(HERE)]
    import torch
    import _vitpkg
    V, O = _vitpkg.load_package(), _vitpkg.load_oracle()
    assert os.path.basename(V.LIB_PATH) == "libviterbi_general.so", V.LIB_PATH
    assert torch.cuda.is_available()
    V.initialize()
    data, bad = Data(O), 0
    for ge in (0, 1):
        msgs = [m for m in case(V, torch, data, 768, ge) if m]
        bad += bool(msgs)
        print("%s fb=768 ge=%d %s" % ("FAIL" if msgs else "ok  ", ge, "; ".join(msgs)), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
