"""CPU-only: MSC time interleaving (include/viterbi_amd.h, "From the CIF stream") as a model independent of the library -
the forward interleaver as EN 300 401 clause 12 states it and a numpy de-interleaver of a CIF ring - pinned by its
properties, among them the one the whole-MSC recipe rests on.  tests/test_gpu_ti.py uses the same model as its
reference."""
import subprocess

import numpy as np

# F[k] = k with its 4 bits reversed
F = np.array([0, 8, 4, 12, 2, 10, 6, 14, 1, 9, 5, 13, 3, 11, 7, 15], np.int64)
CU = 64  # bits (= soft bytes) per capacity unit; sub-channels start at whole CUs


def interleave(frames, fill=0):
    """the transmitter: logical frames 0 ... N-1 of one sub-channel, (N, L) bytes -> CIFs 0 ... N+14, (N+15, L): byte i
    of CIF r = byte i of logical frame r - F[i mod 16]; a byte whose frame lies outside 0 ... N-1 is `fill`"""
    frames = np.asarray(frames, np.uint8)
    N, L = frames.shape
    r, i = np.meshgrid(np.arange(N + 15), np.arange(L), indexing="ij")
    src = r - F[i % 16]
    ok = (src >= 0) & (src < N)
    cif = np.full((N + 15, L), fill, np.uint8)
    cif[ok] = frames[src[ok], i[ok]]
    return cif


def periodic_cif(base, nrows):
    """the transmitter's CIFs 0 ... nrows-1 for the endless stream of logical frames base[n mod len(base)], frames before 0
    included: byte i of CIF r = base[(r - F[i mod 16]) mod len(base)][i] - one period of rows, repeated.  A call with
    frame 0 at row 0 gives frame n = base[n mod len(base)].  (Cheap rings of many frames for the GPU tests and bench.)"""
    base = np.asarray(base, np.uint8)
    nb, L = base.shape
    i = np.arange(L)
    period = base[(np.arange(nb)[:, None] - F[i % 16][None, :]) % nb, i[None, :]]
    return np.tile(period, ((nrows + nb - 1) // nb, 1))[:nrows]


def deinterleave(ring, first_row, col, ncols, nframes):
    """the receiver (these calls): byte i of frame n = ring row (first_row + n + F[i mod 16]) mod nrows, column col + i"""
    ring = np.asarray(ring, np.uint8)
    i = np.arange(ncols)
    rows = (first_row + np.arange(nframes)[:, None] + F[i % 16][None, :]) % ring.shape[0]
    return ring[rows, col + i[None, :]]


def place_in_ring(cif, nrows, first_row, col, row_bytes, rng, poison=None):
    """CIF rows 0 ... R-1 into ring rows (first_row + r) mod nrows at columns [col, col + L); every other byte of the ring
    is `poison` (random bytes if None)"""
    R, L = cif.shape
    assert R <= nrows and col + L <= row_bytes
    ring = (rng.integers(0, 256, (nrows, row_bytes), dtype=np.uint8) if poison is None
            else np.full((nrows, row_bytes), poison, np.uint8))
    ring[(first_row + np.arange(R)) % nrows, col:col + L] = cif
    return ring


def msc_cif(subchannels, width):
    """sub-channels (start CU, (N, L_k) logical frames) -> CIF rows (N+15, width): each interleaved on its own, with i
    counted from its own first byte, and placed at column CU*start"""
    n = subchannels[0][1].shape[0]
    cif = np.zeros((n + 15, width), np.uint8)
    for start, frames in subchannels:
        cif[:, CU * start:CU * start + frames.shape[1]] = interleave(frames)
    return cif


# ---- tests ----------------------------------------------------------------------------------------------------------

def test_f_is_the_4_bit_reversal():
    for k in range(16):
        assert F[k] == int(format(k, "04b")[::-1], 2)
    assert sorted(F.tolist()) == list(range(16))


def test_interleave_then_deinterleave_is_the_identity():
    rng = np.random.default_rng(1)
    for n, L in ((1, 1), (3, 17), (40, 100), (20, 64 * 3 + 5)):
        frames = rng.integers(0, 256, (n, L), dtype=np.uint8)
        cif = interleave(frames)
        assert np.array_equal(deinterleave(cif, 0, 0, L, n), frames)
        # the same rows in a ring that wraps, at an odd column of odd-width rows
        for nrows, first in ((n + 15, n + 14), (n + 40, n + 33)):
            ring = place_in_ring(cif, nrows, first, 3, L + 8, rng)
            assert np.array_equal(deinterleave(ring, first, 3, L, n), frames)
    # byte i of a CIF holds 16 different logical frames over any 16 consecutive i: the spread the code relies on
    frames = np.repeat(np.arange(32, dtype=np.uint8)[:, None], 16, axis=1)
    assert sorted(interleave(frames)[20].tolist()) == list(range(5, 21))


def test_a_receiver_may_start_at_its_first_cif():
    """frame 0 lies in CIFs 0 ... 15 alone, so a call whose frame 0 is the first CIF received is complete.  CIFs 0 ... 14
    also carry bytes of the 15 frames before frame 0 (here `fill`): those frames are the incomplete ones, and a call
    starting at CIF 0 never addresses them."""
    rng = np.random.default_rng(2)
    frames = rng.integers(0, 255, (20, 48), dtype=np.uint8)
    cif = interleave(frames, fill=255)
    assert (cif[:15] == 255).any() and not (cif[15:20] == 255).any()
    assert np.array_equal(deinterleave(cif[:16], 0, 0, 48, 1), frames[:1])  # the first 16 CIFs give frame 0


def test_periodic_cif_is_the_interleaved_periodic_stream():
    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, (7, 37), dtype=np.uint8)
    n = 5 * 7 + 3
    cif = periodic_cif(base, n + 15)
    assert np.array_equal(cif[15:n], interleave(np.tile(base, (6, 1))[:n])[15:n])
    assert np.array_equal(deinterleave(cif, 0, 0, 37, n), np.tile(base, (6, 1))[:n])


def test_one_whole_msc_deinterleave_serves_every_subchannel():
    """sub-channels at random CU-aligned starts, each interleaved with its own byte count: one de-interleave of the
    whole MSC width gives every sub-channel's logical frames at column 64*start"""
    rng = np.random.default_rng(3)
    for _ in range(10):
        n = int(rng.integers(1, 6))
        sizes = rng.integers(1, 40, 3)                     # sub-channel lengths in bytes (any, not whole CUs)
        starts, pos = [], int(rng.integers(0, 3))
        for s in sizes:
            starts.append(pos)
            pos += (int(s) + CU - 1) // CU + int(rng.integers(0, 3))
        width = CU * pos + int(rng.integers(0, 50))
        subs = [(st, rng.integers(0, 256, (n, int(sz)), dtype=np.uint8)) for st, sz in zip(starts, sizes)]
        whole = deinterleave(msc_cif(subs, width), 0, 0, width, n)
        for st, frames in subs:
            assert np.array_equal(whole[:, CU * st:CU * st + frames.shape[1]], frames)


def test_a_start_off_the_16_column_grid_breaks_the_whole_msc_property():
    """the property needs starts that are multiples of 16 columns (whole CUs are): a sub-channel at column 8 is
    recovered by its own de-interleave (col = 8) and not by the whole-width one"""
    rng = np.random.default_rng(4)
    n, L, start = 4, 100, 8
    frames = rng.integers(0, 256, (n, L), dtype=np.uint8)
    cif = np.zeros((n + 15, 128), np.uint8)
    cif[:, start:start + L] = interleave(frames)
    assert np.array_equal(deinterleave(cif, 0, start, L, n), frames)
    assert not np.array_equal(deinterleave(cif, 0, 0, 128, n)[:, start:start + L], frames)
    cif[:, 16:16 + L] = interleave(frames)  # a start of 16 columns is on the grid
    assert np.array_equal(deinterleave(cif, 0, 0, 128, n)[:, 16:16 + L], frames)


NEW_EXPORTS = ("vit_time_deinterleave_dev", "vit_decode_punctured_ti_dev", "vit_dabplus_ti_superframes_dev")


def test_ti_exports(V):
    out = subprocess.check_output(["nm", "-D", "--defined-only", V.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in NEW_EXPORTS:
        assert name in exported and name in V.EXPORTS


def test_ti_calls_fail_loudly(V):
    """without a device: VIT_ERR_NO_DEVICE; with one, a NULL ring is VIT_ERR_ARG - nothing is launched either way"""
    import ctypes as C
    import torch
    want = 1 if torch.cuda.is_available() else 2  # VIT_ERR_ARG / VIT_ERR_NO_DEVICE
    L = V.lib()
    p = V.punct_profile([(774, 0xFFFFFFFF)])
    assert L.vit_time_deinterleave_dev(None, 0, 2304, None, 4, None) == want
    assert L.vit_decode_punctured_ti_dev(None, 0, None, 768, 4, C.byref(p), 128, None) == want
    assert L.vit_dabplus_ti_superframes_dev(None, 0, C.byref(p), 128, None, None, None, None, 24, 4, None) == want
    if want == 2:
        assert "gfx950" in V.last_error()
    assert C.sizeof(V.CifRing) == 24 and V.CifRing.first_row.offset == 20
