"""GPU: MSC time de-interleaving (vit_time_deinterleave_dev, vit_decode_punctured_ti_dev, vit_dabplus_ti_superframes_dev)
against the model of tests/test_ti_host.py, the numpy depuncturer of tests/test_punct_host.py, the CPU oracle and the
existing punctured calls on host-de-interleaved input - byte-exact."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch  # noqa: F401  (torch's runtime first, as when the whole suite is collected)

from test_dab_host import fire_ok_model, scramble
from test_gpu_dab import dabplus_superframes, dabplus_symbols, decodable_segments
from test_gpu_punctured import oracle, random_segments, soft_frames
from test_punct_host import depuncture, fic_segments, puncture
from test_ti_host import CU, deinterleave, interleave, periodic_cif, place_in_ring

pytestmark = pytest.mark.gpu

KERNELS = [0, 1, 2, 3]  # auto, wave-per-frame, packed, latency
GUARD = 64
POISON = 0xA5


def ceil_div(a, b):
    return -(-a // b)


# The launch geometry of csrc/vit_ti.hip, mirrored so that the tests below can assert that a workgroup's run of frames
# takes more than one 16-frame iteration - the steady state in which iteration k+1's rows overwrite the LDS slots that
# iteration k read, behind the prefetch issued during iteration k.
def standalone_windows(ncols):
    n0 = ceil_div(ncols, 1024)
    return ceil_div(ncols, ceil_div(ceil_div(ncols, n0), 16) * 16)


def fused_windows(framebits):
    T = framebits + 6
    return ceil_div(T, ceil_div(T, ceil_div(T, 200)))


def iterations_per_run(torch, nframes, nwin):
    """16-frame iterations of a workgroup's run: runs of max(16, ceil(nframes*nwin / (4*CUs)) rounded up to 16) frames"""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    return max(1, ceil_div(ceil_div(nframes * nwin, 4 * cus), 16))


def dev_ring(ring, offset=1):
    """host ring (nrows, row_bytes) -> a contiguous device view starting `offset` bytes into a fresh allocation"""
    flat = np.ascontiguousarray(ring, np.uint8).reshape(-1)
    buf = torch.full((offset + flat.size + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    buf[offset:offset + flat.size] = torch.from_numpy(flat).cuda()
    return buf[offset:offset + flat.size].view(ring.shape)


def ring_of_frames(rng, punct, nrows, first_row, col, extra):
    """punctured logical frames (N, P) -> interleaved CIF rows placed in a ring of nrows rows of col + P + extra bytes,
    poison everywhere else"""
    cif = interleave(punct)
    return place_in_ring(cif, nrows, first_row, col, col + punct.shape[1] + extra, rng, poison=POISON)


# ---- standalone -----------------------------------------------------------------------------------------------------

def run_standalone(V, torch, ring, first_row, col, ncols, nframes, out_offset=3):
    d_ring = dev_ring(ring)
    buf = torch.full((out_offset + nframes * ncols + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    V.time_deinterleave_dev(d_ring, first_row, col, ncols, buf[out_offset:], nframes)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:out_offset] == 0xEE).all() and (got[out_offset + nframes * ncols:] == 0xEE).all()  # guards
    return got[out_offset:out_offset + nframes * ncols].reshape(nframes, ncols)


def poisoned_ring(rng, nrows, row_bytes, first_row, col, ncols, nframes):
    """random bytes in the call's nframes + 15 rows and its columns, poison everywhere else"""
    ring = np.full((nrows, row_bytes), POISON, np.uint8)
    rows = (first_row + np.arange(nframes + 15)) % nrows
    ring[rows, col:col + ncols] = rng.integers(0, 256, (nframes + 15, ncols), dtype=np.uint8)
    return ring


@pytest.mark.parametrize("ncols", [1, 15, 17, 2304, 55296])
def test_standalone_against_the_model(V, torch_cuda, ncols):
    """rings of 16, 17 and about 100 rows whose call rows wrap, an odd col and odd row_bytes, nframes 1 and nrows - 15;
    guard bytes after the output stay; the poison outside the call's rows and columns never shows"""
    torch = torch_cuda
    rng = np.random.default_rng(ncols)
    for nrows in (16, 17, 101):
        for nframes in sorted({1, nrows - 15}):
            first_row = nrows - 5  # rows first_row ... nrows-1, then 0 ...
            col, row_bytes = 7, 7 + ncols + 4 + ncols % 2  # odd row_bytes
            assert row_bytes % 2 == 1
            ring = poisoned_ring(rng, nrows, row_bytes, first_row, col, ncols, nframes)
            got = run_standalone(V, torch, ring, first_row, col, ncols, nframes)
            assert np.array_equal(got, deinterleave(ring, first_row, col, ncols, nframes)), (ncols, nrows, nframes)


@pytest.mark.parametrize("ncols,nframes", [(17, 5003), (2304, 12007), (55296, 701)])
def test_standalone_large_batch(V, torch_cuda, ncols, nframes):
    """thousands of frames, the ring wrapping.  At 2304 and 55296 columns every workgroup's run takes at least two
    16-frame iterations (row slots rewritten, rows prefetched during the expansion), and the last run and its last
    iteration are partial."""
    torch = torch_cuda
    rng = np.random.default_rng(ncols + 1)
    if ncols >= 2304:
        assert iterations_per_run(torch, nframes, standalone_windows(ncols)) >= 2
    nrows, first_row, col = nframes + 15 + 20, nframes, 5
    ring = poisoned_ring(rng, nrows, col + ncols + 2, first_row, col, ncols, nframes)
    got = run_standalone(V, torch, ring, first_row, col, ncols, nframes)
    assert np.array_equal(got, deinterleave(ring, first_row, col, ncols, nframes))


def test_standalone_restores_interleaved_frames(V, torch_cuda):
    """end to end: logical frames through the transmitter's interleaver, back through the call"""
    torch = torch_cuda
    rng = np.random.default_rng(9)
    frames = rng.integers(0, 256, (300, 333), dtype=np.uint8)
    ring = ring_of_frames(rng, frames, 400, 390, 11, 3)
    assert np.array_equal(run_standalone(V, torch, ring, 390, 11, 333, 300), frames)


# ---- fused decode ---------------------------------------------------------------------------------------------------

def run_ti(V, torch, d_ring, first_row, col, framebits, n, segs, erasure=128, kernel=0, ge=False):
    d_out = torch.full((n, (framebits + 7) // 8), 0xEE, dtype=torch.uint8, device="cuda")
    old_k, old_ge = V.set_kernel(kernel), V.set_renorm_ge(ge)
    try:
        V.decode_punctured_ti_dev(d_ring, first_row, col, d_out, framebits, n, segs, erasure)
        torch.cuda.synchronize()
    finally:
        V.set_kernel(old_k)
        V.set_renorm_ge(old_ge)
    return d_out.cpu().numpy()


def run_punctured(V, torch, punct, framebits, n, segs, erasure=128, kernel=0, ge=False):
    d_out = torch.full((n, (framebits + 7) // 8), 0xEE, dtype=torch.uint8, device="cuda")
    old_k, old_ge = V.set_kernel(kernel), V.set_renorm_ge(ge)
    try:
        V.decode_punctured_dev(torch.from_numpy(np.ascontiguousarray(punct)).cuda(), d_out, framebits, n, segs, erasure)
        torch.cuda.synchronize()
    finally:
        V.set_kernel(old_k)
        V.set_renorm_ge(old_ge)
    return d_out.cpu().numpy()


@pytest.mark.parametrize("framebits", [768, 288, 2304])
def test_fused_decode(V, O, torch_cuda, framebits):
    """FIC-shaped (768 bits: P = 2304 = 36 CU) and random profiles, every kernel, both comparators: the fused call equals
    the oracle's decode of the depunctured frames and vit_decode_punctured_dev on host-de-interleaved input"""
    torch = torch_cuda
    rng = np.random.default_rng(framebits + 21)
    n = 45
    for ge in (False, True):
        segs = fic_segments() if framebits == 768 and not ge else random_segments(rng, framebits)
        punct = puncture(soft_frames(O, n, framebits, seed=framebits + ge), segs, framebits)
        P = punct.shape[1]
        nrows, first_row, col = n + 15 + 6, n + 2, 64 * 3 + 1
        ring = ring_of_frames(rng, punct, nrows, first_row, col, 5)
        host_deint = deinterleave(ring, first_row, col, P, n)
        assert np.array_equal(host_deint, punct)
        want = oracle(O, framebits, punct, segs, 128, ge=ge)
        d_ring = dev_ring(ring)
        for kernel in KERNELS:
            got = run_ti(V, torch, d_ring, first_row, col, framebits, n, segs, kernel=kernel, ge=ge)
            assert np.array_equal(got, want), (framebits, ge, kernel)
            assert np.array_equal(run_punctured(V, torch, host_deint, framebits, n, segs, kernel=kernel, ge=ge), want)


@pytest.mark.parametrize("erasure", [0, 255])
def test_fused_erasure_values(V, O, torch_cuda, erasure):
    torch = torch_cuda
    rng = np.random.default_rng(erasure + 5)
    framebits, n = 768, 40
    segs = random_segments(rng, framebits, nseg=4)
    punct = puncture(soft_frames(O, n, framebits, seed=6), segs, framebits)
    ring = ring_of_frames(rng, punct, n + 15, 3, 0, 0)
    want = oracle(O, framebits, punct, segs, erasure)
    assert np.array_equal(run_ti(V, torch, dev_ring(ring), 3, 0, framebits, n, segs, erasure=erasure), want)


def test_fused_packed_kernel_batch(V, O, torch_cuda):
    """2496 FIC-shaped frames (above 2048: the packed kernel under auto), 96 distinct frames repeated, in a ring that
    wraps"""
    torch = torch_cuda
    rng = np.random.default_rng(31)
    framebits, base_n, reps = 768, 96, 26
    segs = fic_segments()
    base = puncture(soft_frames(O, base_n, framebits, seed=31), segs, framebits)
    want = oracle(O, framebits, base, segs, 128)
    punct = np.tile(base, (reps, 1))
    n = base_n * reps
    assert n > 2048
    nrows, first_row, col = n + 15 + 9, n + 1, 65
    ring = ring_of_frames(rng, punct, nrows, first_row, col, 1)
    d_ring = dev_ring(ring)
    for kernel in (0, 2):
        got = run_ti(V, torch, d_ring, first_row, col, framebits, n, segs, kernel=kernel)
        assert np.array_equal(got.reshape(reps, base_n, -1), np.broadcast_to(want, (reps,) + want.shape)), kernel
    got = run_punctured(V, torch, deinterleave(ring, first_row, col, punct.shape[1], n), framebits, n, segs)
    assert np.array_equal(got.reshape(reps, base_n, -1), np.broadcast_to(want, (reps,) + want.shape))


def test_fused_runs_of_several_iterations(V, O, torch_cuda):
    """9691 FIC-shaped frames (96 distinct ones, periodic) in a ring that wraps: every workgroup's run takes at least two
    16-frame iterations, and the last run and its last iteration are partial.  Every kernel under auto and packed equals
    the oracle, and so does vit_decode_punctured_dev on the frames themselves."""
    torch = torch_cuda
    rng = np.random.default_rng(41)
    framebits, base_n, n = 768, 96, 9691
    assert iterations_per_run(torch, n, fused_windows(framebits)) >= 2
    segs = fic_segments()
    base = puncture(soft_frames(O, base_n, framebits, seed=41), segs, framebits)
    want = np.tile(oracle(O, framebits, base, segs, 128), (ceil_div(n, base_n), 1))[:n]
    nrows, first_row, col = n + 15 + 9, n + 1, 65
    ring = place_in_ring(periodic_cif(base, n + 15), nrows, first_row, col, col + base.shape[1] + 1, rng, poison=POISON)
    d_ring = dev_ring(ring)
    for kernel in (0, 2):
        assert np.array_equal(run_ti(V, torch, d_ring, first_row, col, framebits, n, segs, kernel=kernel), want), kernel
    frames = np.tile(base, (ceil_div(n, base_n), 1))[:n]
    assert np.array_equal(run_punctured(V, torch, frames, framebits, n, segs), want)


# ---- whole CIF ------------------------------------------------------------------------------------------------------

def test_whole_cif_two_paths(V, O, torch_cuda):
    """three sub-channels with different profiles and lengths at CU-aligned starts of every row.  Path A: one whole-width
    vit_time_deinterleave_dev, then one vit_decode_punctured_varlen_dev table (sym_offset = n*width + 64*startCU);
    path B: one vit_decode_punctured_ti_dev per sub-channel.  Both equal the oracle."""
    torch = torch_cuda
    rng = np.random.default_rng(55)
    n = 30
    subs = []  # (framebits, segs, start CU, punct)
    pos = 2
    for fb in (768, 1536, 288):
        segs = fic_segments() if fb == 768 else decodable_segments(rng, fb)
        punct = puncture(soft_frames(O, n, fb, seed=fb + 3), segs, fb)
        subs.append((fb, segs, pos, punct))
        pos += (punct.shape[1] + CU - 1) // CU + 1
    width = CU * pos + 7
    cif = np.zeros((n + 15, width), np.uint8)
    for fb, segs, start, punct in subs:
        cif[:, CU * start:CU * start + punct.shape[1]] = interleave(punct)
    nrows, first_row = n + 15 + 3, n + 10
    ring = place_in_ring(cif, nrows, first_row, 0, width, rng, poison=POISON)
    d_ring = dev_ring(ring)
    wants = [oracle(O, fb, punct, segs, 128) for fb, segs, _, punct in subs]
    # path A
    d_deint = torch.full((n * width,), 0xEE, dtype=torch.uint8, device="cuda")
    V.time_deinterleave_dev(d_ring, first_row, 0, width, d_deint, n)
    desc = np.zeros(n * 3, V.DESC_DTYPE)
    out_pos, expect = 0, []
    for i in range(n):
        for k, (fb, segs, start, punct) in enumerate(subs):
            d = desc[i * 3 + k]
            d["sym_offset"], d["framebits"], d["reserved"], d["out_offset"] = i * width + CU * start, fb, k, out_pos
            expect.append(wants[k][i])
            out_pos += (fb + 7) // 8
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
    d_prof = torch.from_numpy(V.profiles_bytes([s[1] for s in subs])).cuda()
    d_out = torch.full((out_pos,), 0x5A, dtype=torch.uint8, device="cuda")
    V.decode_punctured_varlen_dev(d_deint, d_out, d_desc, desc.size, 1536, d_prof, 3)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), np.concatenate(expect))
    # path B
    for k, (fb, segs, start, punct) in enumerate(subs):
        assert np.array_equal(run_ti(V, torch, d_ring, first_row, CU * start, fb, n, segs), wants[k]), k


# ---- DAB+ -----------------------------------------------------------------------------------------------------------

def run_dabplus(V, torch, nsf, rsdims, call):
    d_work = torch.full((nsf, 120 * rsdims), 0xEE, dtype=torch.uint8, device="cuda")
    d_out = torch.full((nsf, 110 * rsdims), 0xA5, dtype=torch.uint8, device="cuda")
    d_ret = torch.full((nsf,), 0x7777, dtype=torch.int32, device="cuda")
    d_fire = torch.full((nsf + 1,), 0xEE, dtype=torch.uint8, device="cuda")
    call(d_work, d_out, d_ret, d_fire[:nsf])
    torch.cuda.synchronize()
    f = d_fire.cpu().numpy()
    assert f[nsf] == 0xEE
    return d_work.cpu().numpy(), d_out.cpu().numpy(), d_ret.cpu().numpy(), f[:nsf]


@pytest.mark.parametrize("rsdims", [1, 24, 48])
def test_dabplus_from_the_ring(V, O, torch_cuda, rsdims):
    """d_work, d_rs_out, d_ret and d_fire_ok equal vit_dabplus_punctured_superframes_dev on the de-interleaved input"""
    torch = torch_cuda
    rng = np.random.default_rng(200 + rsdims)
    fb = 192 * rsdims
    nsf = 6
    _, sf = dabplus_superframes(rng, nsf, rsdims)
    sym = dabplus_symbols(O, rng, sf, rsdims, ["clean", "3dB", "junk", "flip", "3dB", "clean"])
    segs = decodable_segments(rng, fb)
    punct = puncture(sym, segs, fb)
    P = punct.shape[1]
    nrows, first_row, col = 5 * nsf + 15 + 4, 5 * nsf + 1, 64 * 5
    ring = ring_of_frames(rng, punct, nrows, first_row, col, 3)
    host_deint = deinterleave(ring, first_row, col, P, 5 * nsf)
    assert np.array_equal(host_deint, punct)
    d_ring, d_deint = dev_ring(ring), torch.from_numpy(host_deint).cuda()
    got = run_dabplus(V, torch, nsf, rsdims, lambda w, o, r, f: V.dabplus_ti_superframes_dev(
        d_ring, first_row, col, segs, w, o, r, rsdims, nsf, d_fire_ok=f))
    ref = run_dabplus(V, torch, nsf, rsdims, lambda w, o, r, f: V.dabplus_punctured_superframes_dev(
        d_deint, segs, w, o, r, rsdims, nsf, d_fire_ok=f))
    for g, r in zip(got, ref):
        assert np.array_equal(g, r), rsdims
    work_ref = scramble(O.decode_batch(fb, depuncture(punct, segs, fb, 128), nthreads=8), fb).reshape(nsf, -1)
    assert np.array_equal(got[0], work_ref) and np.array_equal(got[3], fire_ok_model(work_ref))
    assert got[3][0] == 1 and got[2][0] == 0  # the clean superframe


def test_dabplus_from_the_ring_runs_of_several_iterations(V, O, torch_cuda):
    """180 superframes at RSDims 24 (6 distinct ones, periodic): 900 frames, every workgroup's run at least two 16-frame
    iterations.  All four outputs equal vit_dabplus_punctured_superframes_dev on the de-interleaved input, and d_work
    and the fire flags equal the oracle's decode and the model."""
    torch = torch_cuda
    rng = np.random.default_rng(300)
    rsdims, base_sf, nsf = 24, 6, 180
    fb = 192 * rsdims
    assert iterations_per_run(torch, 5 * nsf, fused_windows(fb)) >= 2
    _, sf = dabplus_superframes(rng, base_sf, rsdims)
    sym = dabplus_symbols(O, rng, sf, rsdims, ["clean", "3dB", "flip", "3dB", "clean", "junk"])
    segs = decodable_segments(rng, fb)
    base = puncture(sym, segs, fb)
    reps = nsf // base_sf
    nrows, first_row, col = 5 * nsf + 15 + 2, 7, 64
    ring = place_in_ring(periodic_cif(base, 5 * nsf + 15), nrows, first_row, col, col + base.shape[1] + 3, rng,
                         poison=POISON)
    d_ring, d_deint = dev_ring(ring), torch.from_numpy(np.tile(base, (reps, 1))).cuda()
    got = run_dabplus(V, torch, nsf, rsdims, lambda w, o, r, f: V.dabplus_ti_superframes_dev(
        d_ring, first_row, col, segs, w, o, r, rsdims, nsf, d_fire_ok=f))
    ref = run_dabplus(V, torch, nsf, rsdims, lambda w, o, r, f: V.dabplus_punctured_superframes_dev(
        d_deint, segs, w, o, r, rsdims, nsf, d_fire_ok=f))
    for g, r in zip(got, ref):
        assert np.array_equal(g, r)
    work_ref = scramble(O.decode_batch(fb, depuncture(base, segs, fb, 128), nthreads=8), fb).reshape(base_sf, -1)
    assert np.array_equal(got[0], np.tile(work_ref, (reps, 1)))
    assert np.array_equal(got[3], np.tile(fire_ok_model(work_ref), reps))


# ---- arguments, streams ---------------------------------------------------------------------------------------------

def test_argument_errors(V, torch_cuda):
    """every rule is VIT_ERR_ARG and writes nothing; nframes = 0 is VIT_OK"""
    torch = torch_cuda
    L = V.lib()
    d_ring = torch.zeros((40, 2400), dtype=torch.uint8, device="cuda")
    d = torch.full((1 << 20,), 0x33, dtype=torch.uint8, device="cuda")
    d_ret = torch.full((4,), 0x33, dtype=torch.int32, device="cuda")
    ptr, s = C.c_void_p(d.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = V.punct_profile(fic_segments())
    bad_p = V.punct_profile([(773, 0xFFFFFFFF)])
    p_dab = V.punct_profile([(4614, 0xFFFFFFFF)])  # RSDims 24: 4608 + 6 steps, P = 18456 > 2400 columns

    def ring(**kw):
        r = V.cif_ring(d_ring, 0)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    def calls(r, nframes, prof=p, col=0):
        rr = None if r is None else C.byref(r)
        return [L.vit_time_deinterleave_dev(rr, col, 2304, ptr, nframes, s),
                L.vit_decode_punctured_ti_dev(rr, col, ptr, 768, nframes, C.byref(prof), 128, s)]

    cases = [(None, 1), (ring(d_base=None), 1), (ring(first_row=40), 1), (ring(first_row=41), 1),
             (ring(), 26), (ring(nrows=16), 2)]
    for r, nframes in cases:
        assert calls(r, nframes) == [1, 1], (r and (r.nrows, r.first_row), nframes)
        assert "bad arguments" in V.last_error()
    assert calls(ring(), 25, col=97) == [1, 1]           # col + ncols > row_bytes
    assert calls(ring(row_bytes=2303), 1) == [1, 1]
    assert calls(ring(), 1, col=(1 << 64) - 1) == [1, 1]  # wraps
    assert L.vit_decode_punctured_ti_dev(C.byref(ring()), 0, ptr, 768, 1, C.byref(bad_p), 128, s) == 1
    assert L.vit_decode_punctured_ti_dev(C.byref(ring()), 0, ptr, 768, 1, None, 128, s) == 1
    for r, nsf in ((None, 1), (ring(d_base=None), 1), (ring(first_row=40), 1), (ring(), 6)):
        assert L.vit_dabplus_ti_superframes_dev(None if r is None else C.byref(r), 0, C.byref(p_dab), 128, ptr, ptr,
                                                C.c_void_p(d_ret.data_ptr()), None, 24, nsf, s) == 1
    big = torch.zeros((60, 18456), dtype=torch.uint8, device="cuda")
    assert L.vit_dabplus_ti_superframes_dev(C.byref(V.cif_ring(big, 0)), 1, C.byref(p_dab), 128, ptr, ptr,
                                            C.c_void_p(d_ret.data_ptr()), None, 24, 1, s) == 1  # one column too many
    assert L.vit_dabplus_ti_superframes_dev(C.byref(V.cif_ring(big, 0)), 0, None, 128, ptr, ptr,
                                            C.c_void_p(d_ret.data_ptr()), None, 24, 1, s) == 1  # no profile
    # empty batches: OK, nothing written
    assert calls(ring(), 0) == [0, 0]
    assert L.vit_dabplus_ti_superframes_dev(C.byref(ring()), 0, C.byref(p_dab), 128, ptr, ptr,
                                            C.c_void_p(d_ret.data_ptr()), ptr, 24, 0, s) == 0
    torch.cuda.synchronize()
    assert bool((d == 0x33).all()) and bool((d_ret == 0x33).all())
    with pytest.raises(ValueError):
        V.cif_ring(d_ring[:, 1:], 0)  # not contiguous


def test_two_threads_alternate_fused_and_punctured_calls(V, O, torch_cuda):
    """two threads, each on its own streams, alternating vit_decode_punctured_ti_dev and vit_decode_punctured_dev
    batches of different sizes: the shared scratch buffer's reuse stays ordered"""
    torch = torch_cuda
    rng = np.random.default_rng(77)
    cases = []
    for fb, n in ((768, 2100), (2304, 61), (288, 700)):
        segs = fic_segments() if fb == 768 else random_segments(rng, fb)
        base_n = min(n, 64)
        base = puncture(soft_frames(O, base_n, fb, seed=fb), segs, fb)
        reps = (n + base_n - 1) // base_n
        punct = np.tile(base, (reps, 1))[:n]
        want = np.tile(oracle(O, fb, base, segs, 128), (reps, 1))[:n]
        ring = ring_of_frames(rng, punct, n + 15 + 5, n + 3, 64, 2)
        cases.append((fb, n, segs, dev_ring(ring), n + 3, torch.from_numpy(punct).cuda(), want))
    errs = []

    def work(tid):
        try:
            streams = [torch.cuda.Stream(), torch.cuda.Stream()]
            outs = []
            for rep in range(8):
                st = streams[rep & 1]
                fb, n, segs, d_ring, first_row, d_p, want = cases[(tid + rep) % len(cases)]
                with torch.cuda.stream(st):
                    d_out = torch.zeros((n, (fb + 7) // 8), dtype=torch.uint8, device="cuda")
                    if (rep + tid) % 2 == 0:
                        V.decode_punctured_ti_dev(d_ring, first_row, 64, d_out, fb, n, segs, stream=st.cuda_stream)
                    else:
                        V.decode_punctured_dev(d_p, d_out, fb, n, segs, 128, stream=st.cuda_stream)
                    outs.append((d_out, want, fb, rep))
            torch.cuda.synchronize()
            for d_out, want, fb, rep in outs:
                if not np.array_equal(d_out.cpu().numpy(), want):
                    errs.append((tid, fb, rep))
        except Exception as e:  # noqa: BLE001
            errs.append((tid, repr(e)))

    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
